"""GPU tests of the bit-reproducible training mode (include/coper_hip.h: coper_train_config.deterministic).

Model dimensions are tests/test_gpu_train.py::_CASES; dropout and batch statistics are on as tests/test_gpu_train_csr.py::_md sets them.
The batches are built so that the order of every sum matters: e1 from five ids (one batch kind has ONE e1), rel from two ids, sampled
lookup rows that repeat an id with different labels.  Every bit comparison is unconditional.

Which sampled case reaches which route of the step (coper_train.hip, struct Step):
  score_dh_fused = true   d % 4 == 0 and L <= 8192: every sampled case below but the next two
  score_dh_fused = false  `lookup_narrow_F` (d = 77: k_tr_score_loss + k_tr_score_bwd<false>; three channels, so Conv1BN's sums
                          take the layout for 256 % C != 0) and `cpg_linear` at L = 8193 (k_tr_score_loss + k_tr_dh_gather4)
  dense_scorer_bwd = true  every sampled case that runs (B * |E| * 4 <= 512 MiB), `cpg_linear_e20k` / `plain_e41k` with several LDS
                           stretches of the S row among them
  dense_scorer_bwd = false the mode refuses it: test_flag_and_refusals"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from tests.test_gpu_train import _CASES

pytestmark = pytest.mark.gpu

_SEED = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _md(name):
    md = dict(cdata._COMMON)
    md.update(_CASES[name])
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=0.003)
    return md


def _model(md, params, deterministic, chunk=0):
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in params.items()})
    m.train_init(seed=_SEED, one_vs_all_chunk=chunk, deterministic=deterministic)
    return m


def _batch(md, route, B, L, seed, one_e1=False):
    """route: "sampled" (lookup_values + e2_multi [B, L]), "dense" (e2_multi [B, |E|]) or "csr" (id lists + lab_row)."""
    rng = np.random.default_rng(seed)
    E, R = md["num_ent"], md["num_rel"]
    ids = rng.choice(E, 5, replace=False)
    e1 = ids[rng.integers(0, 1 if one_e1 else 5, B)].astype(np.int64)
    rel = rng.choice(R, 2, replace=False)[rng.integers(0, 2, B)].astype(np.int64)
    if route == "sampled":
        lookup = rng.integers(0, E, (B, L)).astype(np.int32)
        labels = np.zeros((B, L), np.float32)
        labels[:, 0] = 1.0
        labels[rng.random((B, L)) < 0.05] = 1.0
        if L >= 4:      # an id three times in its row, another twice, with different labels
            lookup[:, 1] = lookup[:, 0]
            lookup[:, L - 1] = lookup[:, 0]
            lookup[:, 3] = lookup[:, 2]
            labels[:, 1], labels[:, L - 1], labels[:, 2], labels[:, 3] = 0.0, 1.0, 1.0, 0.0
        return dict(e1=e1, rel=rel, lookup_values=lookup, e2_multi=labels)
    rows = [np.nonzero(rng.random(E) < 0.05)[0] for _ in range(30)]
    rows[1] = np.zeros(0, np.int64)
    lab_row = rng.integers(0, 30, B)
    if route == "dense":
        dense = np.zeros((B, E), np.float32)
        for b, r in enumerate(lab_row):
            dense[b, rows[r]] = 1.0
        return dict(e1=e1, rel=rel, e2_multi=dense, lookup_values=np.zeros((B, 0), np.int32))
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return dict(e1=e1, rel=rel, lab_indptr=indptr, lab_idx=np.concatenate(rows).astype(np.int64), lab_row=lab_row.astype(np.int64))


def _outputs(m, loss):
    """Everything a step leaves behind, as host arrays: loss, gradients, the norm (a double), variables, slots, powers."""
    out = {"loss": loss.cpu().numpy().copy()}
    for leaf in m.trainable_leaves():
        g, gn = m.train_grad(leaf)
        out["grad/" + leaf] = g.cpu().numpy()
        out["global_norm"] = np.float64(gn)
    for k, v in m._tensors.items():
        out["var/" + k] = v.cpu().numpy().copy()
    slots, powers = m.optimizer_state()
    for leaf, parts in slots.items():
        for i, part in enumerate(parts):
            out["slot%d/%s" % (i, leaf)] = np.array(part)
    for k, v in powers.items():
        out["power/" + k] = np.float64(v)
    return out


def _assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k, float(np.abs(x.astype(np.float64) - y).max()))


def _bits_case(name, route, B, L=37, chunk=0, one_e1=False):
    md = _md(name)
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    a, b = _model(md, p0, True, chunk), _model(md, p0, True, chunk)
    assert a.train_deterministic == 1
    # the train-mode forward without the update: loss, logits and h
    batch = _batch(md, route, B, L, 400, one_e1)
    fa = a.train_forward(batch, want_predictions=True, want_h=True)
    fb = b.train_forward(batch, want_predictions=True, want_h=True)
    fa2 = a.train_forward(batch, want_predictions=True, want_h=True)
    for x, y, z in zip(fa, fb, fa2):
        assert torch.equal(x, y) and torch.equal(x, z)
    for step in range(3):
        batch = _batch(md, route, B, L, 400 + step, one_e1)
        if step == 2:
            saved = {k: v.clone() for k, v in a._tensors.items()}
            saved_opt = a.optimizer_state()
        oa = _outputs(a, a.train_step(batch))
        ob = _outputs(b, b.train_step(batch))
        _assert_same_bits(oa, ob, "step %d, two handles" % step)
        if step == 0:
            assert np.array_equal(oa["loss"], fa[0].cpu().numpy())      # (the forward drew this step's masks)
    # handle A back to the state in front of the last step, five times: the same step again
    for rep in range(5):
        a.load_parameters({k: v.clone() for k, v in saved.items()})
        a.load_optimizer_state(*saved_opt)
        _assert_same_bits(_outputs(a, a.train_step(batch)), oa, "repeat %d from the restored state" % rep)
    a.close()
    b.close()


# the served variants: g_linear, g_MLP with batch norm, generated conv, concat_rel, plain ConvE (stacked; and static layers that are not:
# generated conv with a static dense layer, concat_rel, a g_MLP conv generator), looked-up dense layer, looked-up conv + dense
_VARIANTS = ["cpg_linear", "cpg_mlp_bn", "cpg_conv_fc", "cpg_linear_concat", "plain", "cpg_conv_static_fc", "lookup", "lookup_conv"]


@pytest.mark.parametrize("B", [1, 77, 300])
@pytest.mark.parametrize("route", ["sampled", "dense", "csr"])
@pytest.mark.parametrize("name", _VARIANTS)
def test_bits_across_handles_and_repeats(name, route, B):
    """B = 77 is no multiple of 64; 300 is five row blocks of the default mode's column sums and several workgroups per column.
    |E| = 211 is one CSR chunk; test_bits_chunked_csr has several."""
    _bits_case(name, route, B)


@pytest.mark.parametrize("name", ["cpg_linear", "plain", "lookup"])
def test_bits_with_one_e1_for_the_whole_batch(name):
    """Every sample adds to the same embedding row."""
    _bits_case(name, "sampled", 77, one_e1=True)


@pytest.mark.parametrize("name,chunk", [("cpg_linear", 128), ("plain", 128), ("cpg_mlp_bn", 128), ("cpg_wide", 256)])
def test_bits_chunked_csr(name, chunk):
    """|E| = 211 as 128 + 83, |E| = 700 (d = 200) as 256 + 256 + 188."""
    _bits_case(name, "csr", 77, chunk=chunk)


@pytest.mark.parametrize("name,route", [("cpg_linear_c32", "sampled"), ("cpg_linear_c32", "dense"), ("cpg_wide", "sampled"), ("cpg_wide", "dense")])
def test_bits_wide_shapes(name, route):
    """C = 32: 288 filter-gradient columns, beyond one 256-column block; d = 200: the products span several tiles and cut K."""
    _bits_case(name, route, 77)


@pytest.mark.parametrize("name,B,L", [("lookup_narrow_F", 77, 37), ("cpg_linear", 24, 8193), ("cpg_linear_e20k", 77, 37), ("plain_e41k", 77, 37),
                                      ("cpg_linear", 300, 1)])
def test_bits_sampled_routes(name, B, L):
    """Both sides of score_dh_fused and the large-|E| side of the dense scorer backward (the module docstring says which is which)."""
    _bits_case(name, "sampled", B, L=L)


def test_bits_across_processes():
    """Fresh processes, one after the other: two plain ones and one with COPER_TRAIN_ONE_STREAM=1 print the same digest."""
    child = os.path.join(ROOT, "tests", "train_deterministic_child.py")
    digests = []
    for extra in ({}, {}, {"COPER_TRAIN_ONE_STREAM": "1"}):
        env = {k: v for k, v in os.environ.items() if k != "COPER_TRAIN_ONE_STREAM"}
        env.update(extra)
        run = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-4000:]
        digests.append([ln for ln in run.stdout.splitlines() if ln.startswith("DIGEST ")][-1])
    assert digests[0] == digests[1] == digests[2], digests


def _rel_err(a, b, floor):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor)


@pytest.mark.parametrize("route", ["sampled", "csr"])
@pytest.mark.parametrize("name", ["cpg_linear", "plain", "cpg_mlp_bn", "cpg_conv_fc", "cpg_linear_concat", "lookup"])
def test_deterministic_step_matches_oracle(name, route):
    """deterministic = 1 against the float64 oracle over two steps, each held to the step-0 bounds of
    tests/test_gpu_train.py::_train_step_case as tests/test_gpu_train_csr.py::_check_against_oracle restates them (the oracle restarts
    from the device's variables before the second step).  CSR labels in chunks of 128."""
    from oracle import coper_train_oracle as T
    md = _md(name)
    B, L, E = 48, 37, md["num_ent"]
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = _model(md, p0, True, 128 if route == "csr" else 0)
    ref = {k: np.array(v, np.float64) for k, v in p0.items()}
    opt = T.AMSGrad(T.trainable_names(md), ref, lr=md["learning_rate"], clip=5.0)
    for step in range(2):
        batch = _batch(md, route, B, L, 500 + step)
        if route == "csr":
            dense = np.zeros((B, E), np.float32)
            for b, r in enumerate(batch["lab_row"]):
                dense[b, batch["lab_idx"][batch["lab_indptr"][r]:batch["lab_indptr"][r + 1]]] = 1.0
            ob = dict(e1=batch["e1"], rel=batch["rel"], lookup=None, labels=dense)
        else:
            ob = dict(e1=batch["e1"], rel=batch["rel"], lookup=batch["lookup_values"], labels=batch["e2_multi"])
        if step > 0:
            for k in ref:
                ref[k] = m._tensors[k].cpu().numpy().reshape(np.shape(ref[k])).astype(np.float64)
        loss_o, grads_o, gn_o = T.train_step(ref, md, ob, opt, seed=_SEED, step=step, momentum=md["batch_norm_momentum"])
        loss = float(m.train_step(batch).cpu()[0])
        print("step %d loss %.9g oracle %.9g" % (step, loss, loss_o))
        assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (step, loss, loss_o)
        dg = {}
        for leaf in T.trainable_names(md):
            g, gn = m.train_grad(leaf)
            g = g.cpu().numpy().reshape(grads_o[leaf].shape)
            err = _rel_err(g, grads_o[leaf], 1e-3 * gn_o)
            print("  %-40s rel err %.3g" % (leaf, err))
            assert err < 2e-4, (step, leaf, err)
            dg[leaf] = np.abs(g - grads_o[leaf]).max()
        print("  norm %.9g oracle %.9g" % (gn, gn_o))
        assert abs(gn - gn_o) < 1e-4 * gn_o
        for leaf, want in ref.items():
            if leaf == "conv1_bias":      # (exact gradient 0 under batch statistics: nothing to compare, as there)
                continue
            got = m._tensors[leaf].cpu().numpy().reshape(np.shape(want))
            lr_t = md["learning_rate"] * 0.32
            tol = 2e-5 + 1e-5 * np.abs(want).max() + 2.0 * lr_t * 0.1 * dg.get(leaf, 0.0) / 1e-8
            if leaf == "Conv1BN/moving_mean" and "conv1_bias" in ref:
                bias = m._tensors["conv1_bias"].cpu().numpy().reshape(-1)
                tol += np.abs(bias - np.reshape(ref["conv1_bias"], -1)).max()
            assert np.abs(got - want).max() < tol, (step, leaf, np.abs(got - want).max(), tol)
    m.close()


def test_flag_and_refusals():
    import ctypes as C
    from coper_amd import _lib
    from coper_amd._lib import CoperError
    from coper_amd.models import ConvE
    md = _md("cpg_linear")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    assert m._lib.coper_train_deterministic(m._h) == -5      # no training state: -COPER_ESTATE
    with pytest.raises(CoperError):
        m.train_deterministic
    m.train_init(seed=_SEED)
    assert m.train_deterministic == 0
    m.train_init(seed=_SEED, deterministic=True)
    assert m.train_deterministic == 1
    with pytest.raises(CoperError, match="deterministic") as bad:
        m.train_init(seed=_SEED, deterministic=2)
    assert bad.value.code == 1      # COPER_EINVAL
    m.close()
    # an ent_emb that is not 16-byte aligned: routes chosen by alignment sum in another order -- refused, before anything is launched
    m = ConvE(md, device="cuda:0")
    params = {k: torch.as_tensor(np.array(v, np.float32)).to("cuda:0") for k, v in p0.items()}
    E, d = md["num_ent"], md["ent_emb_size"]
    pad = torch.zeros(E * d + 1, device="cuda:0", dtype=torch.float32)
    pad[1:] = params["ent_emb"].reshape(-1)
    params["ent_emb"] = pad[1:].view(E, d)
    assert params["ent_emb"].data_ptr() % 16 == 4
    m.load_parameters(params)
    m.train_init(seed=_SEED, deterministic=True)
    for route in ("sampled", "csr"):
        with pytest.raises(CoperError, match="16-byte aligned") as bad:
            m.train_step(_batch(md, route, 8, 5, seed=1))
        assert bad.value.code == 7      # COPER_EUNSUPPORTED
    m.close()
    # sampled labels past the dense scorer backward's 512 MiB: the default mode's route there is float atomics
    md = dict(_md("cpg_linear"), num_ent=1048583, ent_emb_size=12, emb_h=3, emb_w=4, conv_num_channels=3, conv_filter_height=2, conv_filter_width=2)
    B = 129
    assert B * md["num_ent"] * 4 > 512 * 1024 * 1024
    m = _model(md, cdata.synthetic_params(md, seed=21, ent_std=0.1), True)
    with pytest.raises(CoperError, match="512 MiB") as bad:
        m.train_step(_batch(md, "sampled", B, 5, seed=1))
    assert bad.value.code == 7 and "deterministic" in str(bad.value)
    m.close()


@pytest.mark.parametrize("route", ["sampled", "dense", "csr"])
def test_default_and_deterministic_modes_agree_within_the_oracle_bounds(route):
    """One step of a default-mode handle and of a deterministic one from the same state: loss, gradients and norm within the bounds
    test_deterministic_step_matches_oracle holds either of them to against the oracle (not bit for bit)."""
    md = _md("cpg_mlp_bn")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    a, b = _model(md, p0, False), _model(md, p0, True)
    batch = _batch(md, route, 77, 37, seed=900)
    la, lb = float(a.train_step(batch).cpu()[0]), float(b.train_step(batch).cpu()[0])
    assert abs(la - lb) < 2e-5 * max(1.0, abs(la)), (la, lb)
    gn = a.train_grad("ent_emb")[1]
    for leaf in a.trainable_leaves():
        (ga, na), (gb, nb) = a.train_grad(leaf), b.train_grad(leaf)
        assert _rel_err(gb.cpu().numpy(), ga.cpu().numpy(), 1e-3 * gn) < 2e-4, leaf
        assert abs(na - nb) < 1e-4 * na
    a.close()
    b.close()
