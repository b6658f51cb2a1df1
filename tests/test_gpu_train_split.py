"""GPU tests of the step in three calls (include/coper_hip.h: coper_train_backward | coper_train_grads_export | coper_train_apply;
DESIGN.md 6.3).  Model dimensions are tests/test_gpu_train.py::_CASES, batches those of tests/test_gpu_train_deterministic.py::_batch
(B = 24 ... 48, L = 37), the float64 oracle is oracle/coper_train_oracle.py and the tolerances are the step-0 bounds of
tests/test_gpu_train.py::_train_step_case (tests/split_common.py states them once)."""
import ctypes as C

import numpy as np
import pytest
import torch

from coper_amd import _lib, data as cdata
from tests import split_common as S
from tests.test_gpu_train_deterministic import _assert_same_bits, _batch, _outputs

pytestmark = pytest.mark.gpu

_ROUTES = ["fused", "backward+apply", "backward+export+apply"]
# (model, label form): a generated dense layer, plain ConvE on dense 1-vs-all labels, a g_MLP generator on sparse labels, the looked-up
# table (absent rows), d = 77 (leaves whose length is no multiple of 4, unfused scorer), a 7.4 M-element leaf (two sweeps of the export grid)
_BITS_CASES = [("cpg_linear", "sampled"), ("plain", "dense"), ("cpg_mlp_bn", "csr"), ("lookup", "sampled"), ("lookup_narrow_F", "sampled"),
               ("cpg_wide", "sampled")]


def _model(md, p0, deterministic, seed=S.SEED):
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=seed, clip_norm=S.CLIP, deterministic=deterministic)
    return m


def _update(m, route, batch):
    """One update by `route` -> the loss tensor"""
    if route == "fused":
        return m.train_step(batch)
    loss = m.train_backward(batch)
    if route == "backward+apply":
        m.train_apply()
    else:
        m.train_apply(m.train_grads_export(), 1.0)
    return loss


@pytest.mark.parametrize("name,form", _BITS_CASES)
def test_split_step_is_the_fused_step_bit_for_bit(name, form):
    """Deterministic mode, three handles from one state, three updates: coper_train_step, backward + apply(NULL), backward + export +
    apply(flat, 1) leave the same bytes in the loss, every gradient, the norm, every variable and moving statistic, every slot, the
    powers and the step counter."""
    md = S.md_for(name)
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    ms = [_model(md, p0, True) for _ in _ROUTES]
    for step in range(3):
        batch = _batch(md, form, 40, 37, 400 + step)
        outs = [_outputs(m, _update(m, route, batch).clone()) for m, route in zip(ms, _ROUTES)]
        for route, o in zip(_ROUTES[1:], outs[1:]):
            _assert_same_bits(o, outs[0], "update %d, %s" % (step, route))
    for m in ms:
        m.close()


@pytest.mark.parametrize("route", _ROUTES)
@pytest.mark.parametrize("name,form", _BITS_CASES)
def test_every_route_matches_the_oracle_in_default_mode(name, form, route):
    """Default mode, one update from identical variables: loss, gradients, norm and variables by the step-0 bounds."""
    md = S.md_for(name)
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = _model(md, p0, False)
    ref, opt = S.new_oracle(md, p0)
    batch = S.batch(md, form, 40, 37, 400)
    loss_o, grads_o = S.oracle_backward(ref, md, batch, S.SEED, 0)
    _, gn_o = S.oracle_update(ref, opt, [grads_o])
    loss = float(_update(m, route, batch).cpu()[0])
    print("loss %.9g oracle %.9g" % (loss, loss_o))
    assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o))
    got, gn = {}, None
    for leaf in grads_o:
        g, gn = m.train_grad(leaf)
        got[leaf] = g.cpu().numpy()
    dg = S.check_grads(got, grads_o, gn_o, route)
    print("norm %.9g oracle %.9g" % (gn, gn_o))
    assert abs(gn - gn_o) < 1e-4 * gn_o
    S.check_variables(md, {k: v.cpu().numpy() for k, v in m._tensors.items()}, ref, dg, route)
    m.close()


@pytest.mark.parametrize("name", ["cpg_linear", "lookup_narrow_F", "cpg_wide"])
def test_flat_vector_layout_slices_and_pads(name):
    md = S.md_for(name)
    m = _model(md, cdata.synthetic_params(md, seed=21, ent_std=0.1), True)
    layout, total = m.train_grads_layout()
    assert list(layout) == [k for k in m._specs if not k.endswith(("moving_mean", "moving_variance"))]      # coper_param_spec order
    end = 0
    for leaf, (off, n) in layout.items():
        assert off % 64 == 0 and off >= end and n == m._tensors[leaf].numel(), (leaf, off, n, end)
        end = off + n
    assert total == (end + 63) // 64 * 64
    m.train_backward(_batch(md, "sampled", 24, 37, 400))
    # (NaN in front: whatever the export does not write would show)
    flat = m.train_grads_export(torch.full((total + 64,), float("nan"), device="cuda:0")[:total]).cpu().numpy()
    covered = np.zeros(total, bool)
    for leaf, (off, n) in layout.items():
        g, _ = m.train_grad(leaf)
        assert flat[off:off + n].tobytes() == g.cpu().numpy().tobytes(), leaf
        covered[off:off + n] = True
    assert np.all(flat[~covered] == 0.0) and (~covered).sum() == total - sum(n for _, n in layout.values())
    # accumulate: twice the gradient, pads still 0
    acc = m.train_grads_export(torch.as_tensor(flat).cuda(), accumulate=True).cpu().numpy()
    assert acc.tobytes() == (flat + flat).tobytes()
    m.close()


def test_absent_rows_of_the_looked_up_table_export_as_zeros_and_add_nothing():
    md = S.md_for("lookup")
    m = _model(md, cdata.synthetic_params(md, seed=21, ent_std=0.1), True)
    layout, total = m.train_grads_layout()
    off, n = layout["fc_weights"]
    rowlen = n // md["num_rel"]
    b1, b2 = _batch(md, "sampled", 24, 37, 400), _batch(md, "sampled", 24, 37, 401)
    b1["rel"] = np.arange(24) % 2             # relations {0, 1}
    b2["rel"] = 2 + np.arange(24) % 2         # relations {2, 3}
    m.train_backward(b1)
    first = m.train_grads_export()
    f1 = first.cpu().numpy().copy()
    rows1 = f1[off:off + n].reshape(md["num_rel"], rowlen)
    assert np.abs(rows1[0]).max() > 0 and np.abs(rows1[1]).max() > 0 and not rows1[2:].any()
    m.train_backward(b2)
    # the table's gradient buffer still holds the first batch's rows 0 and 1: the second backward wrote rows 2 and 3 only
    f2 = m.train_grads_export().cpu().numpy()
    rows2 = f2[off:off + n].reshape(md["num_rel"], rowlen)
    assert not rows2[[0, 1, 4, 5]].any() and np.abs(rows2[2]).max() > 0 and np.abs(rows2[3]).max() > 0
    acc = m.train_grads_export(first, accumulate=True).cpu().numpy()
    rows = acc[off:off + n].reshape(md["num_rel"], rowlen)
    assert rows[[0, 1]].tobytes() == rows1[[0, 1]].tobytes()            # the first batch's values, unchanged
    assert rows[[2, 3]].tobytes() == rows2[[2, 3]].tobytes() and not rows[[4, 5]].any()
    assert acc.tobytes() == (f1 + f2).tobytes()
    m.close()


def test_accumulation_of_three_unequal_micro_batches_matches_the_oracle():
    """Dropout and batch statistics on.  The oracle: each micro-batch's gradient with the masks of its own counter value and its own
    batch statistics, the moving statistics moved three times, the mean of the three gradients through one AMSGrad.step."""
    from coper_amd.parallel import DataParallelTrainer
    md = S.md_for("cpg_mlp_bn")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = _model(md, p0, False)
    ref, opt = S.new_oracle(md, p0)
    tr = DataParallelTrainer(m, micro_batches=3)
    batches = [S.batch(md, "sampled", B, 37, 500 + i) for i, B in enumerate((17, 24, 31))]
    losses_o, grads = [], []
    for i, b in enumerate(batches):
        lo, g = S.oracle_backward(ref, md, b, S.SEED, i)
        losses_o.append(lo)
        grads.append(g)
    mean_o, gn_o = S.oracle_update(ref, opt, grads)
    loss = float(tr.step(batches).cpu()[0])
    assert abs(loss - np.mean(losses_o)) < 2e-5 * max(1.0, abs(np.mean(losses_o)))
    dg = S.check_grads(S.flat_slices(tr.flat.cpu().numpy() * np.float32(1.0 / 3.0), tr.layout), mean_o, gn_o, "flat / 3")
    _, gn = m.train_grad("ent_emb")
    print("norm %.9g oracle %.9g" % (gn, gn_o))
    assert abs(gn - gn_o) < 1e-4 * gn_o
    S.check_variables(md, {k: v.cpu().numpy() for k, v in m._tensors.items()}, ref, dg, "update 0")
    tr.step([S.batch(md, "sampled", B, 37, 510 + i) for i, B in enumerate((17, 24, 31))])
    _, powers = m.optimizer_state()
    assert powers["step"] == 6                               # the dropout counter: one per backward
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))      # (coper_train_config holds the betas as floats; the powers start at beta)
    assert abs(powers["beta1_power"] - b1 ** 3) < 1e-12 and abs(powers["beta2_power"] - b2 ** 3) < 1e-12
    m.close()


def test_two_halves_are_the_batch():
    """Without dropout and batch statistics the mean of the two halves' gradients IS the batch's gradient: the accumulated, halved flat
    vector against the ORACLE's gradient of the whole batch."""
    md = S.md_for("cpg_linear", hidden_dropout=0.0, output_dropout=0.0, batch_norm_train_stats=False)
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    from coper_amd.parallel import shard_batch
    m = _model(md, p0, False)
    ref, opt = S.new_oracle(md, p0)
    batch = S.batch(md, "sampled", 48, 37, 400)
    loss_o, grads_o = S.oracle_backward(ref, md, batch, S.SEED, 0)
    _, gn_o = S.oracle_update(ref, opt, [grads_o])
    flat, loss = None, 0.0
    for r in range(2):
        loss += 0.5 * float(m.train_backward(shard_batch(batch, r, 2)).cpu()[0])
        flat = m.train_grads_export(flat, accumulate=r > 0)
    assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o))
    layout, _ = m.train_grads_layout()
    dg = S.check_grads(S.flat_slices(flat.cpu().numpy() * np.float32(0.5), layout), grads_o, gn_o, "flat / 2")
    m.train_apply(flat, 0.5)
    _, gn = m.train_grad("ent_emb")
    assert abs(gn - gn_o) < 1e-4 * gn_o
    S.check_variables(md, {k: v.cpu().numpy() for k, v in m._tensors.items()}, ref, dg, "halves", skip_stats=True)
    m.close()


def test_state_rules():
    md = S.md_for("cpg_linear")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = _model(md, p0, True)
    batch = _batch(md, "sampled", 24, 37, 400)
    ESTATE, EINVAL = 5, 1

    def code(fn, *a):
        with pytest.raises(_lib.CoperError) as e:
            fn(*a)
        return e.value.code

    assert code(m.train_apply) == ESTATE                      # before any backward
    m.train_backward(batch)
    m.train_apply()
    assert code(m.train_apply) == ESTATE                      # twice
    m.train_backward(batch)
    m.train_forward(batch)                                    # zeroes the gradient buffers
    assert code(m.train_apply) == ESTATE
    m.train_backward(batch)
    m.train_step(batch)                                       # a step after a discarded backward works, and discards it
    assert code(m.train_apply) == ESTATE
    layout, total = m.train_grads_layout()
    m.train_backward(batch)
    buf = torch.zeros(total + 8, device="cuda:0")
    assert code(m.train_grads_export, buf[:total - 64]) == EINVAL          # cap too small
    assert code(m.train_grads_export, buf[1:total + 1]) == EINVAL          # misaligned
    flat = m.train_grads_export(buf[:total])
    assert code(m.train_apply, buf[:total - 64]) == EINVAL                 # a wrong n
    assert code(m.train_apply, buf[1:total + 1]) == EINVAL                 # misaligned
    before = {k: v.clone() for k, v in m._tensors.items() if not k.endswith(("moving_mean", "moving_variance"))}
    m.train_apply(flat)                                                    # a refused apply consumed nothing and changed nothing
    assert any(not torch.equal(m._tensors[k], v) for k, v in before.items())
    m.close()


def test_refused_apply_keeps_the_pending_gradients():
    md = S.md_for("cpg_linear")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    a, b = _model(md, p0, True), _model(md, p0, True)
    batch = _batch(md, "sampled", 24, 37, 400)
    _, total = a.train_grads_layout()
    la, lb = a.train_backward(batch).clone(), b.train_backward(batch).clone()
    with pytest.raises(_lib.CoperError):
        a.train_apply(torch.zeros(total - 64, device="cuda:0"))
    a.train_apply()
    b.train_apply()
    _assert_same_bits(_outputs(a, la), _outputs(b, lb), "after a refused apply")
    a.close()
    b.close()


def test_evaluation_between_backward_and_apply_changes_nothing():
    """A ranking pass between the two calls groups its own queries by relation -- other relations than the batch's -- in the workspace
    the step's grouping used: apply reads the backward's snapshot of the counts."""
    md = S.md_for("lookup")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    a, b = _model(md, p0, True), _model(md, p0, True)
    batch = _batch(md, "sampled", 24, 37, 400)
    batch["rel"] = np.arange(24) % 2
    q = cdata.synthetic_queries(md, 40, seed=3)
    q["rel"] = 2 + np.arange(40) % 4
    a.train_step(_batch(md, "sampled", 24, 37, 399))
    b.train_step(_batch(md, "sampled", 24, 37, 399))
    la = a.train_backward(batch).clone()
    a.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
    a.train_apply()
    lb = b.train_backward(batch).clone()
    b.train_apply()
    _assert_same_bits(_outputs(a, la), _outputs(b, lb), "with and without a ranking pass in between")
    a.close()
    b.close()


def test_registering_a_moving_statistic_keeps_the_carried_weight_maximum():
    """coper_train_wmax_carried: an update leaves the dense weights' maximum for the next step's packs; registering a BN moving statistic
    again (what a data-parallel step does after averaging them) keeps it, registering a trainable leaf drops it."""
    md = S.md_for("cpg_linear")
    m = _model(md, cdata.synthetic_params(md, seed=21, ent_std=0.1), False)
    batch = _batch(md, "sampled", 24, 37, 400)
    assert m.train_wmax_carried == 0
    m.train_step(batch)
    assert m.train_wmax_carried == 1
    m._tensors["Conv1BN/moving_mean"].mul_(1.0)      # an in-place torch op: the next call registers the tensor again
    m.train_backward(batch)
    assert m.train_wmax_carried == 1
    m.parameters_changed("FCBN/moving_variance")
    assert m.train_wmax_carried == 1
    m.train_apply()
    assert m.train_wmax_carried == 1
    m.parameters_changed("FCBN/gamma")
    assert m.train_wmax_carried == 0
    m.train_backward(batch)
    m.train_apply(m.train_grads_export(), 1.0)
    assert m.train_wmax_carried == 1
    m.close()
