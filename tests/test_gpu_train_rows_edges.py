"""GPU tests of the deferred-rows mode (coper_amd/csrc/train_rows.h) away from the one operating point of
tests/test_gpu_train_rows.py and tests/test_gpu_train_rows_split.py: a global-norm clip that ACTS (the listed rows' share of the norm
reaches the update through the clip factor alone), scalar and two-trip lane loops (d = 77, d = 288), more listed rows than one pass of
any row kernel's grid (32,768 rows; four slots of k_rows_export at 98,304), row blocks whose vals are 4-byte but not 16-byte aligned,
beta powers late in training (beta1^t subnormal and 0.0) and changed with rows behind, and the statistics kernel past its grid.
References: oracle/coper_train_oracle.py (float64, dense AMSGrad) with the same planted slots, the float64 zero-gradient loop of G.1,
and plain NumPy.  A twin handle with the mode off runs beside the deferred one and is held to the same references.

Bounds (from the project, none from what these kernels give): variables by G.2's law, dev_deferred <= 2 dev_dense + 2e-5 + 1e-5 max|w|;
slots m / v / v_hat of every leaf by the same form WITHOUT the absolute floor, dev_deferred <= 2 dev_dense + 1e-4 max|w| -- the twin
measures the float32 and GEMM rounding of the same run, 1e-4 relative is about a hundred float32 roundings, and a table norm left out
of the clip moves the scale, and with it m, by more than 10 %; zero-gradient rows against the float64 loop by G.1's bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from coper_amd import _lib, data as cdata
from tests.test_gpu_train_rows import (B, E, F32, L, SEED, _batch_below, _gap_batch, _ids, _labels, _loss_close, _md, _model, _oracle,
                                       _oracle_state, _state)

pytestmark = pytest.mark.gpu

TABLES = ("ent_emb", "pred_bias")
E_BIG = 131101                 # odd; rows_grid() is 8,192 workgroups of 4 waves: one pass of a row kernel covers 32,768 rows
BIG_B, BIG_L = 104, 1000       # 104,104 unique rows > 3 * 32,768: the fourth in-flight slot of k_rows_export carries rows
E_STATS = 1048583              # k_rows_stats: 4,096 workgroups of 256 threads = 1,048,576 rows per pass


def _p0(md):
    return cdata.synthetic_params(md, seed=21, ent_std=0.1)


def _planted(p0, seed=9):
    """Slots for every row of both tables: m ~ N(0, 1e-3), v ~ U(1e-9, 1e-5), v_hat = v U(1, 3), float32.  A row that misses one update
    then moves p by about 1e-3 (lr_t m / sqrt(v_hat))."""
    rng = np.random.default_rng(seed)
    out = {}
    for leaf in TABLES:
        shape = np.shape(p0[leaf])
        mm = rng.normal(0, 1e-3, shape).astype(F32)
        vv = rng.uniform(1e-9, 1e-5, shape).astype(F32)
        hh = (vv * rng.uniform(1.0, 3.0, shape)).astype(F32)
        out[leaf] = (mm, vv, hh)
    return out


def _plant_oracle(opt, planted):
    for leaf, (mm, vv, hh) in planted.items():
        assert opt.m[leaf].shape == mm.shape
        opt.m[leaf], opt.v[leaf], opt.vh[leaf] = mm.astype(np.float64), vv.astype(np.float64), hh.astype(np.float64)


def _oracle_step_norm(md, ref, opt, batch, step):
    """_oracle_step with the global gradient norm the oracle's AMSGrad clipped by -> (loss, norm)"""
    from oracle import coper_train_oracle as T
    ob = dict(e1=batch["e1"], rel=batch["rel"], lookup=batch["lookup_values"], labels=batch["e2_multi"])
    loss, _, gn = T.train_step(ref, md, ob, opt, seed=SEED, step=step, momentum=md["batch_norm_momentum"])
    return float(loss), float(gn)


def _pair(md, p0, planted, clip):
    models = {"deferred": _model(md, p0, deferred_rows=True, clip_norm=clip), "dense": _model(md, p0, clip_norm=clip)}
    for m in models.values():
        m.load_optimizer_state(planted)
    return models


def _check_laws(tag, got, want):
    """Every variable and slot of both handles against the oracle's by the two laws of the module docstring."""
    assert set(want) <= set(got["deferred"])
    bad = []
    for key, w in sorted(want.items()):
        dev = {mode: float(np.abs(got[mode][key].reshape(w.shape) - w).max()) for mode in got}
        wmax = float(np.abs(w).max())
        room = 2e-5 + 1e-5 * wmax if key[1] == "p" else 1e-4 * wmax
        print("%s %s/%s: deferred %.3e dense %.3e room %.3e (max |w| %.3e)" % (tag, key[0], key[1], dev["deferred"], dev["dense"], room, wmax))
        if not dev["deferred"] <= 2.0 * dev["dense"] + room:
            bad.append((key, dev, room))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ E.1
CLIP_E1 = 0.1


@functools.lru_cache(maxsize=None)
def _clipped_trajectory(name):
    """The float64 oracle over the six gap batches of G.2 with planted slots and clip 0.1 (needs no GPU) ->
    ([loss], [global norm], final state)"""
    md = _md(name)
    p0 = _p0(md)
    ref, opt = _oracle(md, p0)
    opt.clip = CLIP_E1
    _plant_oracle(opt, _planted(p0))
    steps = [_oracle_step_norm(md, ref, opt, _gap_batch(md, step), step) for step in range(6)]
    return [s[0] for s in steps], [s[1] for s in steps], _oracle_state(ref, opt)


@pytest.mark.parametrize("name", ["cpg_linear", "lookup_narrow_F", "fuzz_d288"])
def test_a_clip_that_acts_at_three_row_layouts(name):
    """G.2's six steps with gaps at clip_norm = 0.1, below half the global norm of every step (asserted on the oracle's norms), with
    planted slots in every row of both tables: the squares k_rows_sumsq adds reach every element through the clip factor.  Row layouts:
    cpg_linear d = 40 (float4, one trip of the lane loop), lookup_narrow_F d = 77 (scalar, two trips), fuzz_d288 d = 288 (float4, two
    trips).  Every variable and slot after the final sync by the two laws; the per-step loss by the non-tight law.  Before this file
    the table rows' share of the gradient norm was untested: at clip 5.0 the factor is 1 whatever the kernel adds.  Measured
    deviations: DESIGN 6.4."""
    md = _md(name)
    p0 = _p0(md)
    losses_o, norms_o, want = _clipped_trajectory(name)
    print("E.1 %s oracle norms %s" % (name, " ".join("%.3f" % g for g in norms_o)))
    assert min(norms_o) > 2.0 * CLIP_E1, norms_o
    models = _pair(md, p0, _planted(p0), CLIP_E1)
    losses = []
    for step in range(6):
        batch = _gap_batch(md, step)
        for mode, m in models.items():
            losses.append((float(m.train_step(batch).cpu()[0]), losses_o[step]))
    st = models["deferred"].train_row_stats()
    assert st["rows_behind"] > 0 and st["max_gap"] == 6, st
    _check_laws("E.1 " + name, {mode: _state(m) for mode, m in models.items()}, want)      # (first: it says which leaf and slot)
    for got_loss, want_loss in losses:
        _loss_close(got_loss, want_loss)
    for m in models.values():
        m.close()


# ------------------------------------------------------------------------------------------------ E.3
CLIP_E3 = 0.01


@functools.lru_cache(maxsize=None)
def _big_md():
    md = _md("cpg_linear")
    md["num_ent"] = E_BIG
    return md


@functools.lru_cache(maxsize=None)
def _big_p0():
    return _p0(_big_md())


def _big_batch(md, seed):
    """B = 104, L = 1000 over a seeded permutation of the ids: 104,000 lookup entries and 104 e1, all distinct -- 104,104 unique rows."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(md["num_ent"])
    n = BIG_B * BIG_L
    return dict(e1=perm[n:n + BIG_B].astype(np.int64), rel=rng.integers(0, md["num_rel"], BIG_B),
                lookup_values=perm[:n].reshape(BIG_B, BIG_L).astype(np.int32), e2_multi=_labels(rng, BIG_B, BIG_L))


def _batch_rows(batch):
    return np.unique(np.concatenate([np.asarray(batch["e1"]).reshape(-1), np.asarray(batch["lookup_values"]).reshape(-1)]).astype(np.int64))


def _big_schedule(md):
    return [_gap_batch(md, 0), _big_batch(md, 1), _gap_batch(md, 2), _big_batch(md, 2)]


@functools.lru_cache(maxsize=None)
def _big_trajectory():
    """The float64 oracle over the four updates of E.3 (needs no GPU) -> ([loss], [global norm], final state)"""
    md, p0 = _big_md(), _big_p0()
    ref, opt = _oracle(md, p0)
    opt.clip = CLIP_E3
    _plant_oracle(opt, _planted(p0))
    steps = [_oracle_step_norm(md, ref, opt, batch, step) for step, batch in enumerate(_big_schedule(md))]
    return [s[0] for s in steps], [s[1] for s in steps], _oracle_state(ref, opt)


def test_more_rows_than_one_pass_of_any_grid():
    """|E| = 131,101, planted slots, clip 0.01 (acting: asserted on the oracle's norms).  Updates: a small gap batch, a batch of 104,104
    unique rows, a small one, a second big one.  The big batches take k_rows_catch_up, k_rows_sumsq and k_rows_update through four
    passes of their grid-stride loops; update 2 grows the id lists while the list of update 1 is owed its re-zero; update 3 re-zeroes
    104,104 rows (a claim bit left set would cost update 4 a listed row: rows_last_step is checked per update); the final sync strides
    over |E| and is the only update the never-named rows get.  Per update: the loss law and rows_last_step; before the sync the
    statistics against step words kept on the host; after it every variable and slot against the oracle by the two laws.  Measured
    deviations: DESIGN 6.4."""
    md, p0 = _big_md(), _big_p0()
    batches = _big_schedule(md)
    losses_o, norms_o, want = _big_trajectory()
    print("E.3 oracle norms %s" % " ".join("%.4f" % g for g in norms_o))
    assert min(norms_o) > 2.0 * CLIP_E3, norms_o
    word, now = np.zeros(E_BIG, np.int64), 0
    assert _batch_rows(batches[1]).size == _batch_rows(batches[3]).size == BIG_B * (BIG_L + 1) > 3 * 32768
    models = _pair(md, p0, _planted(p0), CLIP_E3)
    for step, batch in enumerate(batches):
        rows = _batch_rows(batch)
        assert rows[0] >= 0 and rows[-1] < E_BIG
        for mode, m in models.items():
            _loss_close(float(m.train_step(batch).cpu()[0]), losses_o[step])
        assert models["deferred"].train_row_stats()["rows_last_step"] == rows.size, step
        now += 1
        word[rows] = now
    never = int((word == 0).sum())
    print("E.3 never-named rows: %d" % never)
    assert never > 0
    st = models["deferred"].train_row_stats()
    assert st["rows_behind"] == int((word < now).sum()) and st["max_gap"] == int((now - word).max()) == 4, st
    got = {mode: _state(m) for mode, m in models.items()}
    assert models["deferred"].train_row_stats()["rows_behind"] == 0
    _check_laws("E.3", got, want)
    # ... and the never-named rows alone, where the sync's stride is the only thing that reaches them
    idle = word == 0
    for leaf in TABLES:
        for kind in ("p", "m", "v", "vh"):
            w = want[(leaf, kind)]
            dev = {mode: float(np.abs(got[mode][(leaf, kind)].reshape(w.shape)[idle] - w[idle]).max()) for mode in got}
            wmax = float(np.abs(w[idle]).max())
            room = 2e-5 + 1e-5 * wmax if kind == "p" else 1e-4 * wmax
            print("E.3 never-named %s/%s: deferred %.3e dense %.3e room %.3e" % (leaf, kind, dev["deferred"], dev["dense"], room))
            assert dev["deferred"] <= 2.0 * dev["dense"] + room, (leaf, kind, dev, room)
    for m in models.values():
        m.close()


# ------------------------------------------------------------------------------------------------ E.4
def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def _table_grads(m, n_ent, d):
    return m.train_grad("ent_emb")[0].cpu().numpy().reshape(n_ent, d), m.train_grad("pred_bias")[0].cpu().numpy().reshape(n_ent)


def test_export_and_import_past_one_pass():
    """test_export_is_a_copy's assertions on a pending list of 104,104 rows, exported at row_cap = the bound (every id slot used) and at
    row_cap = |E| (26,997 ids of -1 behind the count): all four in-flight slots of k_rows_export carry rows.  Then the block onto a
    second handle that has run three small steps: import(first) -- the gradient buffers equal the block exactly; a one-row import(first)
    -- its re-zero strides over the 104,104 rows, every other row is zero; the big block again -- 104,104 rows are listed (a claim bit
    the strided re-zero left set would keep its row off the list).  No oracle: copies and counts."""
    md, p0 = _big_md(), _big_p0()
    d = md["ent_emb_size"]
    big = _big_batch(md, 1)
    want_ids = _batch_rows(big)
    bound = min(BIG_B * (BIG_L + 1), E_BIG)
    assert want_ids.size == bound
    m = _model(md, p0, deferred_rows=True)
    rs = m.train_rows_layout()[2]
    m.train_rows_backward(big)
    gE, gb = _table_grads(m, E_BIG, d)
    others = np.ones(E_BIG, bool)
    others[want_ids] = False
    assert not gE[others].any() and not gb[others].any()
    blocks = {}
    for cap in (bound, E_BIG):
        # (NaN and 7 in front: whatever the export does not write would show)
        ids0 = torch.full((cap,), 7, device="cuda:0", dtype=torch.int32)
        vals0 = torch.full((cap, rs), float("nan"), device="cuda:0")
        _, ids_t, vals_t, count = m.train_rows_export(False, ids=ids0, vals=vals0)
        ids, vals, n = ids_t.cpu().numpy(), vals_t.cpu().numpy(), int(count.cpu()[0])
        assert n == want_ids.size == m.train_row_stats()["rows_last_step"], cap
        assert np.array_equal(np.sort(ids[:n]), want_ids) and np.all(ids[n:] == -1), cap
        assert _same_bits(vals[:n, :d], gE[ids[:n]]) and _same_bits(vals[:n, d], gb[ids[:n]]), cap
        assert np.abs(vals[:n, :d]).max() > 0 and np.abs(vals[:n, d]).max() > 0
        assert np.all(vals[:n, d + 1:].view(np.uint32) == 0), cap
        blocks[cap] = (ids_t, vals_t, ids, vals, n)
    m.close()

    b = _model(md, p0, deferred_rows=True)
    for step in range(3):
        b.train_step(_gap_batch(md, step))
    ids_t, vals_t, ids, vals, n = blocks[E_BIG]
    b.train_rows_import(ids_t, vals_t, first=True)
    assert b.train_row_stats()["rows_last_step"] == n
    hE, hb = _table_grads(b, E_BIG, d)
    assert _same_bits(hE[ids[:n]], vals[:n, :d]) and _same_bits(hb[ids[:n]], vals[:n, d])
    assert not hE[others].any() and not hb[others].any()
    # one row: the re-zero of the list before strides
    one = int(ids[n - 1])
    one_vals = np.zeros((1, rs), F32)
    one_vals[0, :d + 1] = np.random.default_rng(3).normal(0, 1, d + 1)
    b.train_rows_import(torch.as_tensor(np.array([one], np.int32)).cuda(), torch.as_tensor(one_vals).cuda(), first=True)
    assert b.train_row_stats()["rows_last_step"] == 1
    hE, hb = _table_grads(b, E_BIG, d)
    rest = np.ones(E_BIG, bool)
    rest[one] = False
    assert _same_bits(hE[one], one_vals[0, :d]) and _same_bits(hb[one], one_vals[0, d])
    assert not hE[rest].any() and not hb[rest].any()
    # the big block again: every claim bit was cleared
    ids_t, vals_t, ids, vals, n = blocks[bound]
    b.train_rows_import(ids_t, vals_t, first=True)
    assert b.train_row_stats()["rows_last_step"] == bound
    hE, hb = _table_grads(b, E_BIG, d)
    assert _same_bits(hE[ids[:n]], vals[:n, :d]) and _same_bits(hb[ids[:n]], vals[:n, d])
    assert not hE[others].any() and not hb[others].any()
    b.close()


# ------------------------------------------------------------------------------------------------ E.5
def test_a_vals_block_off_the_16_byte_grid():
    """Float4 tables (d = 40) with a vals block one float past a 16-byte boundary -- the ABI asks for 4-byte alignment -- through the C
    calls themselves: the export gives the bits of the aligned export, the import the gradient bits of the aligned import, and the NaN
    guards on both sides of the block are untouched."""
    md = _md("cpg_linear")
    d = md["ent_emb_size"]
    p0 = _p0(md)
    m = _model(md, p0, deferred_rows=True)
    rs = m.train_rows_layout()[2]
    batch = _gap_batch(md, 0)
    m.train_rows_backward(batch)
    bound = min(B * (L + 1), E)
    _, ids_a, vals_a, count_a = m.train_rows_export(False, ids=torch.full((bound,), 7, device="cuda:0", dtype=torch.int32),
                                                    vals=torch.full((bound, rs), float("nan"), device="cuda:0"))
    n = int(count_a.cpu()[0])
    assert n == _ids(batch).size
    guard = 64
    buf = torch.full((guard + 1 + bound * rs + guard,), float("nan"), device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    vals_ptr = buf.data_ptr() + 4 * (guard + 1)
    assert vals_ptr % 16 == 4
    ids_u = torch.full((bound,), 7, device="cuda:0", dtype=torch.int32)
    count_u = torch.zeros(1, device="cuda:0", dtype=torch.int32)
    _lib.check(m._h, m._lib.coper_train_rows_export(m._h, None, 0, 0, ids_u.data_ptr(), vals_ptr, bound, count_u.data_ptr(), m._stream()))
    host = buf.cpu().numpy()
    block = host[guard + 1:guard + 1 + bound * rs].reshape(bound, rs)
    assert int(count_u.cpu()[0]) == n and np.array_equal(ids_u.cpu().numpy(), ids_a.cpu().numpy())
    assert np.array_equal(block.view(np.uint32), vals_a.cpu().numpy().view(np.uint32))      # (the rows behind the count: NaN on both sides)
    assert np.abs(block[:n, :d + 1]).max() > 0
    assert np.isnan(host[:guard + 1]).all() and np.isnan(host[guard + 1 + bound * rs:]).all()
    gE, gb = _table_grads(m, E, d)
    m.close()
    # the import: aligned, then from the shifted block, onto a fresh handle
    b = _model(md, p0, deferred_rows=True)
    b.train_rows_import(ids_a, vals_a, first=True)
    aE, ab = _table_grads(b, E, d)
    assert _same_bits(aE, gE) and _same_bits(ab, gb) and np.abs(aE).max() > 0
    b._sync_parameters()
    _lib.check(b._h, b._lib.coper_train_rows_import(b._h, ids_u.data_ptr(), vals_ptr, bound, 1, b._stream()))
    assert b.train_row_stats()["rows_last_step"] == n
    uE, ub = _table_grads(b, E, d)
    assert _same_bits(uE, aE) and _same_bits(ub, ab)
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), host.view(np.uint32))
    b.close()


# ------------------------------------------------------------------------------------------------ E.6
def _read_powers(m):
    """coper_train_powers as a plain get (model.optimizer_state() would sync the rows first)."""
    b1, b2 = C.c_double(), C.c_double()
    _lib.check(m._h, m._lib.coper_train_powers(m._h, None, None, None, C.byref(b1), C.byref(b2), None))
    return b1.value, b2.value


def _zero_gradient_run(tag, segments):
    """G.1's set-up (rows 128 .. 256 planted -- 16 rows with v > v_hat, 16 all zero -- and without gradient) over `segments` =
    [(t or None, steps)]: before a segment with t the powers of both handles are set to beta^t.  The float64 loop of dense zero-gradient
    updates starts every segment from the powers the handle reports (which must be the ones set); G.1's bound."""
    md = _md("cpg_linear")
    p0 = _p0(md)
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
    lr, b1, b2, eps = float(F32(md["learning_rate"])), float(F32(0.9)), float(F32(0.999)), float(F32(1e-8))
    models = {mode: _model(md, p0, deferred_rows=mode == "deferred") for mode in ("deferred", "dense")}
    ref = {}
    for leaf in TABLES:
        p = np.asarray(p0[leaf], F32).astype(np.float64).reshape(planted[leaf][0].shape)[lo:]
        ref[leaf] = [p] + [a[lo:].astype(np.float64) for a in planted[leaf]]
    step, behind = 0, []
    for seg, (t, steps) in enumerate(segments):
        powers = None if t is None else dict(beta1_power=b1 ** t, beta2_power=b2 ** t)
        st = models["deferred"].train_row_stats()
        behind.append((st["rows_behind"], st["max_gap"]))
        for m in models.values():
            m.load_optimizer_state(planted if seg == 0 else {}, powers=powers)
        b1p, b2p = _read_powers(models["dense"])
        assert _read_powers(models["deferred"]) == (b1p, b2p)
        if powers is not None:
            assert (b1p, b2p) == (powers["beta1_power"], powers["beta2_power"]), (t, b1p, b2p, powers)
        print("%s segment %d: beta1_power %.6e beta2_power %.6e" % (tag, seg, b1p, b2p))
        for _ in range(steps):
            batch = _batch_below(md, lo, B, L, seed=1000 + step % 16)
            for m in models.values():
                m.train_step(batch)
            step += 1
            for leaf in TABLES:
                p, mm, vv, hh = ref[leaf]
                lr_t = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
                mm, vv = b1 * mm, b2 * vv
                hh = np.maximum(hh, vv)
                p = p - lr_t * mm / (np.sqrt(hh) + eps)
                ref[leaf] = [p, mm, vv, hh]
            b1p, b2p = b1p * b1, b2p * b2
        assert _read_powers(models["deferred"]) == _read_powers(models["dense"]) == (b1p, b2p)
    st = models["deferred"].train_row_stats()
    behind.append((st["rows_behind"], st["max_gap"]))
    got = {mode: _state(m) for mode, m in models.items()}
    assert models["deferred"].train_row_stats()["rows_behind"] == 0
    bad = []
    for leaf in TABLES:
        for kind, w in zip(("p", "m", "v", "vh"), ref[leaf]):
            dev = {mode: float(np.abs(got[mode][(leaf, kind)].reshape((E,) + w.shape[1:])[lo:] - w).max()) for mode in got}
            ulp4 = 4.0 * float(np.spacing(F32(np.abs(w).max())))
            print("%s %s/%s: deferred %.3e dense %.3e (4 ulp %.3e)" % (tag, leaf, kind, dev["deferred"], dev["dense"], ulp4))
            if not dev["deferred"] <= max(dev["dense"], ulp4):
                bad.append((leaf, kind, dev, ulp4))
    assert not bad, bad
    # the all-zero rows keep the exact bits of p
    for leaf in TABLES:
        shape = planted[leaf][0].shape
        p_now = models["deferred"]._tensors[leaf].detach().cpu().numpy().reshape(shape)[lo + 16:lo + 32]
        assert np.array_equal(p_now.view(np.uint32), np.asarray(p0[leaf], F32).reshape(shape)[lo + 16:lo + 32].view(np.uint32))
    for m in models.values():
        m.close()
    assert behind[-1][1] == segments[-1][1], behind      # (the last segment's steps are the gap the final sync closed)
    return behind


@pytest.mark.parametrize("t", [5, 3000, 7000, 8000])
def test_late_beta_powers(t):
    """G.1 at N = 9 with the powers set to beta^t (the float32 betas as doubles): t = 5; t = 3000; t = 7000, where beta1^t is
    subnormal (4.985e-321); t = 8000, where it is exactly 0.0 and its log2 -inf.  RowCatchUp carries the powers as log2 for these.
    Measured deviations: DESIGN 6.4."""
    b1 = float(F32(0.9))
    if t == 7000:
        assert 0.0 < b1 ** t < 2.3e-308
    if t == 8000:
        assert b1 ** t == 0.0
    _zero_gradient_run("E.6 t=%d" % t, [(t, 9)])


def test_powers_changed_with_rows_behind():
    """Three steps from the initial powers, the powers set to beta^3000 while rows 128 .. 256 are three updates behind, three more
    steps: coper_train_powers brings every row current under the OLD powers before it sets the new ones (a catch-up reads the gap's
    learning rates off the current powers), so the reference loop runs three updates under the old powers and three under the new."""
    behind = _zero_gradient_run("E.6 changed", [(None, 3), (3000, 3)])
    assert behind[1][0] > 0 and behind[1][1] == 3, behind      # (rows were behind when the powers were set)


# ------------------------------------------------------------------------------------------------ E.7
def test_row_statistics_past_one_pass():
    """|E| = 1,048,583: seven rows beyond one pass of k_rows_stats's grid (4,096 x 256), all of them behind after one small step."""
    md = _md("cpg_linear")
    md["num_ent"] = E_STATS
    m = _model(md, _p0(md), deferred_rows=True)
    batch = _gap_batch(md, 0)
    m.train_step(batch)
    st = m.train_row_stats()
    assert st == dict(rows_last_step=_ids(batch).size, rows_behind=E_STATS - _ids(batch).size, max_gap=1), st
    m.train_sync_rows()
    st = m.train_row_stats()
    assert st["rows_behind"] == 0 and st["max_gap"] == 0, st
    m.close()
