"""GPU tests of the deferred-rows mode of the sampled training step (include/coper_hip.h "Deferred rows"): rows of
ent_emb / pred_bias that a batch does not name are left alone and brought current later by the closed form of their zero-gradient
AMSGrad updates.  References: a float64 NumPy loop of dense zero-gradient updates (G.1) and oracle/coper_train_oracle.py, whose AMSGrad
is the dense one (G.2, G.5, G.6); a twin handle with the mode off runs beside the deferred one and is held to the same references."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from tests.test_gpu_train import _CASES

pytestmark = pytest.mark.gpu

E = 257          # odd: pred_bias ends in a scalar tail, the last word of the claim bitmap is partial
B, L = 8, 12
SEED = 5
F32 = np.float32


def _md(name, train_stats=False):
    md = dict(cdata._COMMON)
    md.update(_CASES[name])
    md.update(num_ent=E, batch_norm_train_stats=train_stats, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    return md


def _model(md, p0, **kw):
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, F32)) for k, v in p0.items()})
    m.train_init(seed=SEED, **kw)
    return m


def _labels(rng, b, l):
    labels = np.zeros((b, l), F32)
    labels[:, 0] = 1.0
    labels[rng.random((b, l)) < 0.05] = 1.0
    return labels


def _batch_below(md, hi, b, l, seed):
    """A sampled batch whose e1 and lookup ids all lie in [0, hi)."""
    rng = np.random.default_rng(seed)
    return dict(e1=rng.integers(0, hi, b), rel=rng.integers(0, md["num_rel"], b), lookup_values=rng.integers(0, hi, (b, l)).astype(np.int32),
                e2_multi=_labels(rng, b, l))


# id sets of the gap schedules: A in every step (0 .. 7 as e1 only), SB in steps 0 and 4, SC in step 1 only, the rest never
A_E1, A_LK, SB, SC = np.arange(0, 8), np.arange(8, 40), np.arange(40, 80), np.arange(80, 120)


def _gap_batch(md, step, seed=300):
    rng = np.random.default_rng(seed + step)
    lookup = rng.choice(A_LK, (B, L)).astype(np.int32)
    if step in (0, 4):
        lookup[:, 1:4] = rng.choice(SB, (B, 3))
    if step == 1:
        lookup[:, 4:7] = rng.choice(SC, (B, 3))
    e1 = rng.choice(A_E1, B)
    lookup[2, 9] = lookup[2, 8]          # one lookup row carries an id twice
    e1[4] = lookup[4, 10]                # one id is the e1 and a lookup entry of the same sample
    return dict(e1=e1, rel=rng.integers(0, md["num_rel"], B), lookup_values=lookup, e2_multi=_labels(rng, B, L))


def _ids(batch):
    ids = np.concatenate([np.asarray(batch["e1"]).reshape(-1), np.asarray(batch["lookup_values"]).reshape(-1)]).astype(np.int64)
    ids[(ids < 0) | (ids >= E)] = 0      # the clamp of k_tr_conv_fwd / k_tr_score_bwd / k_tr_build_S
    return np.unique(ids)


def _oracle(md, p0):
    from oracle import coper_train_oracle as T
    ref = {k: np.array(v, np.float64) for k, v in p0.items()}
    return ref, T.AMSGrad(T.trainable_names(md), ref, lr=md["learning_rate"], clip=5.0)


def _oracle_step(md, ref, opt, batch, step):
    from oracle import coper_train_oracle as T
    ob = dict(e1=batch["e1"], rel=batch["rel"], lookup=batch["lookup_values"], labels=batch["e2_multi"])
    return T.train_step(ref, md, ob, opt, seed=SEED, step=step, momentum=md["batch_norm_momentum"])[0]


def _state(m):
    """Every variable and every slot of the model as float64 host arrays, keyed (leaf, kind): a sync, then plain reads."""
    m.train_sync_rows()
    slots, _ = m.optimizer_state()
    out = {(k, "p"): t.detach().cpu().numpy().astype(np.float64) for k, t in m._tensors.items()}
    for leaf, parts in slots.items():
        for kind, a in zip(("m", "v", "vh"), parts):
            out[(leaf, kind)] = np.asarray(a, np.float64)
    return out


def _oracle_state(ref, opt):
    out = {(k, "p"): np.asarray(v, np.float64) for k, v in ref.items()}
    for kind, d in (("m", opt.m), ("v", opt.v), ("vh", opt.vh)):
        for leaf, a in d.items():
            out[(leaf, kind)] = np.asarray(a, np.float64)
    return out


def _loss_close(got, want):
    assert abs(got - want) < 2e-4 * max(1.0, abs(want)), (got, want)      # the non-tight law of _train_step_case


# ------------------------------------------------------------------------------------------------ G.1
@pytest.mark.parametrize("N,b,l", [(1, B, L), (9, B, L), (450, 4, 8)])
def test_untouched_rows_follow_the_closed_form_and_the_dense_loop(N, b, l):
    """Rows 128 .. 256 carry planted slots (16 rows with v > v_hat, 16 all zero) and get no gradient for N steps; after a sync they are
    compared with a float64 loop of N dense zero-gradient updates, and so are the same rows of a twin handle with the mode off.  Per
    leaf the deferred deviation may not exceed the larger of the dense twin's and 4 float32 ulps of the largest compared magnitude
    (deferred rounds p once where dense rounds N times, and forms m and v from one rounded power).  N = 450 is past the truncation
    window of C at beta1 = 0.9 (426 terms).  Measured deviations: DESIGN 6.4."""
    md = _md("cpg_linear")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    rng = np.random.default_rng(9)
    lo, d = 128, md["ent_emb_size"]
    planted = {}
    for leaf, shape in (("ent_emb", (E, d)), ("pred_bias", (E,))):
        mm, vv, hh = np.zeros(shape, F32), np.zeros(shape, F32), np.zeros(shape, F32)
        mm[lo:] = rng.normal(0, 1e-3, mm[lo:].shape)
        vv[lo:] = rng.uniform(1e-9, 1e-5, vv[lo:].shape)
        hh[lo:] = vv[lo:] * rng.uniform(1.0, 3.0, vv[lo:].shape)
        hh[lo:lo + 16] = 0.5 * vv[lo:lo + 16]                                   # v > v_hat
        mm[lo + 16:lo + 32] = vv[lo + 16:lo + 32] = hh[lo + 16:lo + 32] = 0     # all zero
        planted[leaf] = (mm, vv, hh)
    models = {}
    for mode in ("deferred", "dense"):
        m = _model(md, p0, deferred_rows=mode == "deferred")
        assert m.train_rows_deferred == (1 if mode == "deferred" else 0)
        m.load_optimizer_state(planted)
        models[mode] = m
    _, powers = models["dense"].optimizer_state()
    for step in range(N):
        batch = _batch_below(md, lo, b, l, seed=1000 + step % 16)
        for m in models.values():
            m.train_step(batch)
    # the float64 loop: lr, the betas and epsilon as the library holds them (floats), the powers as coper_train_powers reported them
    lr, b1, b2, eps = float(F32(md["learning_rate"])), float(F32(0.9)), float(F32(0.999)), float(F32(1e-8))
    want = {}
    for leaf in ("ent_emb", "pred_bias"):
        p = np.asarray(p0[leaf], F32).astype(np.float64).reshape(planted[leaf][0].shape)[lo:]
        mm, vv, hh = (a[lo:].astype(np.float64) for a in planted[leaf])
        b1p, b2p = powers["beta1_power"], powers["beta2_power"]
        for _ in range(N):
            lr_t = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
            mm, vv = b1 * mm, b2 * vv
            hh = np.maximum(hh, vv)
            p = p - lr_t * mm / (np.sqrt(hh) + eps)
            b1p, b2p = b1p * b1, b2p * b2
        want.update({(leaf, "p"): p, (leaf, "m"): mm, (leaf, "v"): vv, (leaf, "vh"): hh})
    got = {mode: _state(m) for mode, m in models.items()}
    assert models["deferred"].train_row_stats()["rows_behind"] == 0
    for key, w in want.items():
        dev = {mode: float(np.abs(got[mode][key].reshape((E,) + w.shape[1:])[lo:] - w).max()) for mode in got}
        ulp4 = 4.0 * float(np.spacing(F32(np.abs(w).max())))
        print("G.1 N=%d %s/%s: deferred %.3e dense %.3e (4 ulp %.3e)" % (N, key[0], key[1], dev["deferred"], dev["dense"], ulp4))
        assert dev["deferred"] <= max(dev["dense"], ulp4), (N, key, dev, ulp4)
    # the all-zero rows keep the exact bits of p
    for leaf in ("ent_emb", "pred_bias"):
        p_now = models["deferred"]._tensors[leaf].detach().cpu().numpy().reshape(planted[leaf][0].shape)[lo + 16:lo + 32]
        assert np.array_equal(p_now.view(np.uint32), np.asarray(p0[leaf], F32).reshape(planted[leaf][0].shape)[lo + 16:lo + 32].view(np.uint32))
    for m in models.values():
        m.close()


# ------------------------------------------------------------------------------------------------ G.2
@pytest.mark.parametrize("name", ["cpg_linear", "plain"])
def test_trajectory_with_gaps_matches_the_training_oracle(name):
    """Six free-running steps on hand-built batches (set A every step, SB in steps 0 and 4, SC in step 1 only -- brought current by the
    final sync alone -- the rest never; ids that are e1 only, a duplicated lookup id, an id that is e1 and lookup entry of one sample),
    then every variable and every slot against the float64 oracle.  Per leaf the deferred deviation is held to twice the dense twin's
    plus _train_step_case's absolute floor; the per-step loss to its non-tight law.  BN takes the moving statistics: under batch
    statistics conv1_bias has an exact gradient of 0 and moves by rounding noise alone on every side (_train_step_case excludes it),
    which says nothing about rows.  Measured deviations: DESIGN 6.4."""
    md = _md(name)
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    ref, opt = _oracle(md, p0)
    models = {"deferred": _model(md, p0, deferred_rows=True), "dense": _model(md, p0)}
    for step in range(6):
        batch = _gap_batch(md, step)
        loss_o = _oracle_step(md, ref, opt, batch, step)
        for mode, m in models.items():
            _loss_close(float(m.train_step(batch).cpu()[0]), loss_o)
    st = models["deferred"].train_row_stats()
    assert st["rows_behind"] > 0 and st["max_gap"] == 6, st      # (the never-named rows; SC is 4 behind)
    got = {mode: _state(m) for mode, m in models.items()}
    want = _oracle_state(ref, opt)
    assert set(want) <= set(got["deferred"])
    for key, w in sorted(want.items()):
        dev = {mode: float(np.abs(got[mode][key].reshape(w.shape) - w).max()) for mode in got}
        floor = 2e-5 + 1e-5 * float(np.abs(w).max())
        print("G.2 %s %s/%s: deferred %.3e dense %.3e floor %.3e" % (name, key[0], key[1], dev["deferred"], dev["dense"], floor))
        assert dev["deferred"] <= 2.0 * dev["dense"] + floor, (key, dev, floor)
    for m in models.values():
        m.close()


# ------------------------------------------------------------------------------------------------ G.3
def _raw_slots(m):
    """The six table slots through coper_train_slot itself (a get syncs in the mode), as host arrays."""
    out = {}
    for leaf in ("ent_emb", "pred_bias"):
        for which in range(3):
            n = C.c_int64()
            m._lib.coper_train_slot(m._h, leaf.encode(), which, None, 0, 0, C.byref(n), m._stream())
            buf = torch.empty(n.value, device=m.device, dtype=torch.float32)
            rc = m._lib.coper_train_slot(m._h, leaf.encode(), which, C.c_void_p(buf.data_ptr()), n.value, 0, C.byref(n), m._stream())
            assert rc == 0
            out[(leaf, which)] = buf.cpu().numpy()
    return out


def _raw_tables(m):
    return {k: m._tensors[k].detach().cpu().numpy().copy() for k in ("ent_emb", "pred_bias")}


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_read_paths_sync_themselves():
    md = _md("cpg_linear")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = _model(md, p0, deferred_rows=True)
    for step in range(3):
        m.train_step(_gap_batch(md, step))
    assert m.train_row_stats()["rows_behind"] > 0
    # a slot get brings the rows current itself: nothing is left for the explicit sync to change
    slots = _raw_slots(m)
    assert m.train_row_stats()["rows_behind"] == 0
    tables = _raw_tables(m)
    m.train_sync_rows()
    _same_bits(slots, _raw_slots(m))
    _same_bits(tables, _raw_tables(m))
    # ... and so does prepare(): encode after it equals encode after an explicit sync and a second prepare
    m.train_step(_gap_batch(md, 3))
    m.train_step(_gap_batch(md, 4))
    assert m.train_row_stats()["rows_behind"] > 0
    q = cdata.synthetic_queries(md, 12, seed=3)
    h1 = m.encode(q["e1"], q["rel"]).cpu().numpy()
    assert m.train_row_stats()["rows_behind"] == 0
    tables = _raw_tables(m)
    m.train_sync_rows()
    m.prepare()
    h2 = m.encode(q["e1"], q["rel"]).cpu().numpy()
    assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32))
    # a second sync changes no bit
    m.train_sync_rows()
    _same_bits(tables, _raw_tables(m))
    m.close()


# ------------------------------------------------------------------------------------------------ G.4
def test_the_steps_table_work_follows_the_batch():
    """rows_last_step is the number of unique clamped ids of the batch; the step's structure is read through the profile interface
    (coper_profile_read of the counts the training step files, include/coper_hip.h): in the mode no whole-buffer zeroing of the two
    tables and k_tr_sumsq / k_tr_amsgrad over every leaf but them; with the mode off both, as always."""
    md = _md("cpg_linear")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m, dense = _model(md, p0, deferred_rows=True), _model(md, p0)
    batches = [_gap_batch(md, 0), _batch_below(md, E, B, L, seed=7), _batch_below(md, 30, B, L, seed=8)]
    batches[1]["lookup_values"][0, 0] = E + 5      # out of range: row 0, as the step's kernels clamp it
    batches[1]["lookup_values"][1, 1] = -3
    batches[1]["e1"][2] = E
    batches[2]["lookup_values"][:, 1] = batches[2]["lookup_values"][:, 0]      # duplicates in every row
    n_leaves = len(m.trainable_leaves())
    for mm in (m, dense):
        mm.profile(True)
    for batch in batches:
        m.train_step(batch)
        dense.train_step(batch)
        assert m.train_row_stats()["rows_last_step"] == _ids(batch).size
        for mm, tables, leaves in ((m, 0, n_leaves - 2), (dense, 1, n_leaves)):
            assert mm.profile_read("train.zero.ent_emb")[1] == tables and mm.profile_read("train.zero.pred_bias")[1] == tables
            assert mm.profile_read("train.zero.rel_emb")[1] == 1
            assert mm.profile_read("train.amsgrad.leaves")[1] == leaves and mm.profile_read("train.sumsq.leaves")[1] == leaves
        for k in ("rezero", "claim", "catch_up", "sumsq", "update"):
            assert m.profile_read("train.rows." + k)[1] == 1 and dense.profile_read("train.rows." + k)[1] == 0, k
        assert m.profile_read("train.rows.sync")[1] == 0
    assert dense.train_row_stats() == dict(rows_last_step=0, rows_behind=0, max_gap=0)
    m.close()
    dense.close()


# ------------------------------------------------------------------------------------------------ G.5
def test_train_forward_in_the_mode():
    md = _md("cpg_linear")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    ref, opt = _oracle(md, p0)
    m = _model(md, p0, deferred_rows=True)
    word, now = np.zeros(E, np.int64), 0      # the step words as this test expects them

    def check_stats():
        st = m.train_row_stats()
        assert st["rows_behind"] == int((word < now).sum()) and st["max_gap"] == int((now - word).max()), (st, now)

    for step in range(3):
        batch = _gap_batch(md, step)
        _loss_close(float(m.train_step(batch).cpu()[0]), _oracle_step(md, ref, opt, batch, step))
        now += 1
        word[_ids(batch)] = now
        check_stats()
    # forward on a batch that names SB (two updates behind) again: the oracle's loss of that batch on the oracle's state
    fb = _gap_batch(md, 4)
    loss_o = _oracle_step(md, copy.deepcopy(ref), copy.deepcopy(opt), fb, 3)
    loss, _, _ = m.train_forward(fb)
    _loss_close(float(loss.cpu()[0]), loss_o)
    word[_ids(fb)] = now       # brought current, nothing advanced: the rows outside the batch are as far behind as they were
    check_stats()
    assert m.train_row_stats()["rows_last_step"] == _ids(fb).size
    # the next step is where the oracle puts it
    batch = _gap_batch(md, 3)
    _loss_close(float(m.train_step(batch).cpu()[0]), _oracle_step(md, ref, opt, batch, 3))
    now += 1
    word[_ids(batch)] = now
    check_stats()
    m.close()


# ------------------------------------------------------------------------------------------------ G.6
def test_refusals_and_order():
    from coper_amd._lib import CoperError
    md = _md("cpg_linear")
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    det = _model(md, p0, deterministic=True)
    with pytest.raises(CoperError) as e:
        det.train_defer_rows(True)
    assert e.value.code == 7
    assert det.train_rows_deferred == 0
    det.close()

    ref, opt = _oracle(md, p0)
    m = _model(md, p0, deferred_rows=True)
    with pytest.raises(CoperError) as e:
        m.train_defer_rows(2)
    assert e.value.code == 1
    step = 0
    for step in range(2):
        batch = _gap_batch(md, step)
        _loss_close(float(m.train_step(batch).cpu()[0]), _oracle_step(md, ref, opt, batch, step))
    sampled = _gap_batch(md, 2)
    dense_labels = np.zeros((B, E), F32)
    dense_labels[np.arange(B), sampled["lookup_values"][:, 0]] = 1.0
    ova = dict(e1=sampled["e1"], rel=sampled["rel"], e2_multi=dense_labels)
    csr = dict(e1=sampled["e1"], rel=sampled["rel"], lab_indptr=np.arange(B + 1, dtype=np.int64),
               lab_idx=sampled["lookup_values"][:, 0].astype(np.int64))
    m.train_grads_layout()
    for call in (lambda: m.train_step(csr), lambda: m.train_step(ova), lambda: m.train_backward(sampled), lambda: m.train_grads_export(),
                 lambda: m.train_apply()):
        with pytest.raises(CoperError, match="deferred-rows mode") as e:
            call()
        assert e.value.code == 7
    # the handle is usable: the next step is where the oracle puts it
    _loss_close(float(m.train_step(sampled).cpu()[0]), _oracle_step(md, ref, opt, sampled, 2))
    assert m.train_row_stats()["rows_behind"] > 0
    # off with rows behind: every row current (against the oracle, never-named rows included), then a dense step
    m.train_defer_rows(False)
    assert m.train_rows_deferred == 0 and m.train_row_stats()["rows_behind"] == 0
    for leaf in ("ent_emb", "pred_bias"):
        w = np.asarray(ref[leaf], np.float64)
        got = m._tensors[leaf].detach().cpu().numpy().reshape(w.shape)      # (a raw read: the mode is off, the tensors are current)
        assert np.abs(got - w).max() < 2e-5 + 5e-5 * np.abs(w).max(), leaf
    m.profile(True)
    batch = _gap_batch(md, 3)
    _loss_close(float(m.train_step(batch).cpu()[0]), _oracle_step(md, ref, opt, batch, 3))
    assert m.profile_read("train.zero.ent_emb")[1] == 1 and m.profile_read("train.rows.claim")[1] == 0      # the dense path
    # ... and on again
    m.train_defer_rows(True)
    batch = _gap_batch(md, 4)
    _loss_close(float(m.train_step(batch).cpu()[0]), _oracle_step(md, ref, opt, batch, 4))
    assert m.profile_read("train.zero.ent_emb")[1] == 0 and m.profile_read("train.rows.claim")[1] == 1
    m.close()


# ------------------------------------------------------------------------------------------------ G.7
def test_the_mode_off_is_untouched():
    """A handle that never enabled the mode (deterministic, so that bits are comparable) gives the bits of a second fresh handle over
    three steps, every variable and slot.  (Against the parent commit's build the same comparison was made once by hand, with
    tools/ab_build.py.)"""
    md = _md("cpg_linear", train_stats=True)
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    states, losses = [], []
    for _ in range(2):
        m = _model(md, p0, deterministic=True)
        losses.append([float(m.train_step(_gap_batch(md, step)).cpu()[0]) for step in range(3)])
        assert m.train_rows_deferred == 0
        states.append({k: v.astype(F32) for k, v in _state(m).items()})
        m.close()
    assert losses[0] == losses[1]
    _same_bits(states[0], states[1])
