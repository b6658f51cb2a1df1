"""GPU tests of the split step of the deferred-rows mode (include/coper_hip.h "Deferred rows: the step in calls"):
coper_train_rows_backward | _export | _import | _apply.  Shapes, batches and references are those of tests/test_gpu_train_rows.py
(|E| = 257, B = 8, L = 12, d = 40; d = 77 for the scalar route): oracle/coper_train_oracle.py through tests/split_common.py, and plain
NumPy.  Every test here fails on a library without the five calls."""
import functools

import numpy as np
import pytest
import torch

from coper_amd import _lib, data as cdata
from coper_amd._lib import CoperError
from tests import split_common as S
from tests.test_gpu_train_rows import (B, E, F32, L, SEED, _batch_below, _gap_batch, _ids, _loss_close, _md, _model, _oracle_state,
                                       _state)

pytestmark = pytest.mark.gpu

TABLES = ("ent_emb", "pred_bias")


def _p0(md):
    return cdata.synthetic_params(md, seed=21, ent_std=0.1)


def _grad(m, leaf):
    return m.train_grad(leaf)[0].cpu().numpy()


def _table_grads(m, d):
    return _grad(m, "ent_emb").reshape(E, d), _grad(m, "pred_bias").reshape(E)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ S.0
@pytest.mark.parametrize("name,rs", [("cpg_linear", 44), ("lookup_narrow_F", 80)])
def test_layout(name, rs):
    """The small vector is the flat vector without the two tables' padded slices, in coper_param_spec order, every leaf at a multiple of
    64 floats; rs = (d + 1 + 3) & ~3; the same with the mode on and off; the two tables are not in it (COPER_EINVAL by name)."""
    md = _md(name)
    d = md["ent_emb_size"]
    assert rs == (d + 4) & ~3 == (d + 1 + 3) & ~3
    got = []
    for deferred in (True, False):
        m = _model(md, _p0(md), deferred_rows=deferred)
        layout, total, stride = m.train_rows_layout()
        flat_layout, flat_total = m.train_grads_layout()
        assert stride == rs
        assert list(layout) == [k for k in flat_layout if k not in TABLES]
        end = 0
        for leaf, (off, n) in layout.items():
            assert off % 64 == 0 and off == end and n == flat_layout[leaf][1], (leaf, off, n, end)
            end = off + (n + 63) // 64 * 64
        assert total == end == flat_total - sum((flat_layout[t][1] + 63) // 64 * 64 for t in TABLES)
        for t in TABLES:
            assert m._lib.coper_train_rows_layout(m._h, t.encode(), None, None, None, None) == 1
        assert m._lib.coper_train_rows_layout(m._h, b"no_such_leaf", None, None, None, None) == 1
        got.append((layout, total, stride))
        m.close()
    assert got[0] == got[1]


# ------------------------------------------------------------------------------------------------ S.1
@pytest.mark.parametrize("name", ["cpg_linear", "lookup_narrow_F"])
def test_export_is_a_copy(name):
    """A batch with a duplicated lookup id, an id that is e1 and a lookup entry, and ids outside [0, E) (row 0, as the step's kernels
    clamp them).  The exported ids are the unique clamped ids, each once; count their number; ids behind it -1; every vals row the bits
    of that row of the dense gradient buffers, pad columns 0; the other rows of the dense gradients 0; the small vector the bits of
    coper_train_grad per leaf, pads 0.  A block one row short of the bound is COPER_EINVAL and costs the pending state nothing."""
    md = _md(name)
    d = md["ent_emb_size"]
    m = _model(md, _p0(md), deferred_rows=True)
    layout, total, rs = m.train_rows_layout()
    batch = _batch_below(md, E, B, L, seed=7)
    batch["e1"][:] = np.arange(100, 100 + B)                # (no row 0 in the batch but through the clamp)
    batch["lookup_values"][batch["lookup_values"] == 0] = 1
    batch["lookup_values"][2, 9] = batch["lookup_values"][2, 8]
    batch["e1"][4] = batch["lookup_values"][4, 10]
    batch["lookup_values"][0, 0] = E + 5
    batch["lookup_values"][1, 1] = -3
    batch["lookup_values"][3, 3] = E - 1                    # row 256: the last bit of the partial claim word
    want_ids = _ids(batch)
    assert want_ids[0] == 0 and want_ids[-1] == E - 1
    m.train_rows_backward(batch)
    bound = min(B * (L + 1), E)
    # (NaN and 7 in front: whatever the export does not write would show)
    small0 = torch.full((total,), float("nan"), device="cuda:0")
    ids0 = torch.full((bound,), 7, device="cuda:0", dtype=torch.int32)
    vals0 = torch.full((bound, rs), float("nan"), device="cuda:0")
    small, ids, vals, count = m.train_rows_export(small0, ids=ids0, vals=vals0)
    small, ids, vals, n = small.cpu().numpy(), ids.cpu().numpy(), vals.cpu().numpy(), int(count.cpu()[0])
    assert n == want_ids.size == m.train_row_stats()["rows_last_step"]
    assert np.array_equal(np.sort(ids[:n]), want_ids) and np.all(ids[n:] == -1)
    gE, gb = _table_grads(m, d)
    assert _same_bits(vals[:n, :d], gE[ids[:n]]) and _same_bits(vals[:n, d], gb[ids[:n]])
    assert np.abs(vals[:n, :d]).max() > 0 and np.abs(vals[:n, d]).max() > 0
    assert np.all(vals[:n, d + 1:].view(np.uint32) == 0)
    others = np.setdiff1d(np.arange(E), want_ids)
    assert not gE[others].any() and not gb[others].any()
    covered = np.zeros(total, bool)
    for leaf, (off, ln) in layout.items():
        assert _same_bits(small[off:off + ln], _grad(m, leaf)), leaf
        covered[off:off + ln] = True
    assert np.all(small[~covered].view(np.uint32) == 0)
    # the allocating form: the block at the backward's bound, the same bits; accumulate doubles the small vector
    small2, ids2, vals2, count2 = m.train_rows_export()
    assert ids2.numel() == bound and tuple(vals2.shape) == (bound, rs) and int(count2.cpu()[0]) == n
    assert np.array_equal(ids2.cpu().numpy(), ids) and _same_bits(vals2.cpu().numpy()[:n], vals[:n]) and _same_bits(small2.cpu().numpy(), small)
    acc = m.train_rows_export(small2, accumulate=True)[0].cpu().numpy()
    assert _same_bits(acc, small + small)
    # small alone (no block) through the C call; the block alone
    assert m._lib.coper_train_rows_export(m._h, small0.data_ptr(), total, 0, None, None, 0, None, m._stream()) == 0
    assert m._lib.coper_train_rows_export(m._h, None, 0, 0, ids0.data_ptr(), vals0.data_ptr(), bound, None, m._stream()) == 0
    assert m._lib.coper_train_rows_export(m._h, None, 0, 0, ids0.data_ptr(), None, bound, None, m._stream()) == 1
    # one row short
    with pytest.raises(CoperError) as e:
        m.train_rows_export(ids=ids0[:bound - 1], vals=vals0[:bound - 1])
    assert e.value.code == 1
    assert m.train_row_stats()["rows_last_step"] == n
    m.train_rows_apply()            # ... the pending state survived it
    with pytest.raises(CoperError) as e:
        m.train_rows_apply()        # ... and is consumed now
    assert e.value.code == 5
    m.close()


# ------------------------------------------------------------------------------------------------ S.2
def _block(rng, rows, rs, d, n, bad_every=0, one_is_E=False):
    """A host-built block of n entries: `rows` in order (distinct), -1 interleaved at every bad_every-th entry, one entry == E; the vals
    rows of bad entries are NaN (an entry that were read would show), the pad columns of good ones 0."""
    ids = np.full(n, -1, np.int32)
    good = np.array([i for i in range(n) if not (bad_every and i % bad_every == 1)], np.int64)
    if one_is_E:
        ids[good[-1]] = E
        good = good[:-1]
    assert good.size == len(rows)
    ids[good] = rows
    vals = np.full((n, rs), np.nan, F32)
    vals[good] = 0.0
    vals[good, :d + 1] = (rng.normal(0, 1, (good.size, d + 1)) * 10.0 ** rng.uniform(-3, 3, (good.size, d + 1))).astype(F32)
    return ids, vals


@pytest.mark.parametrize("name", ["cpg_linear", "lookup_narrow_F"])
def test_import_adds_in_call_order(name):
    """Four host-built blocks of 1, 64, 65 and 257 entries (a wave of the ballot, one entry more, the whole table with row 256) with
    overlapping rows, interleaved -1 entries and one entry == E, imported onto a handle that has run no step (the lists grow from nothing
    and keep what they hold).  After every import the dense gradient buffers equal the float32 sum of the blocks in call order --
    np.float32((a + b) + c) -- exactly, are zero in every other row, rows_last_step is the size of the union, and the bad entries have
    changed nothing (their vals are NaN).  A second `first` import discards the lot."""
    md = _md(name)
    d = md["ent_emb_size"]
    m = _model(md, _p0(md), deferred_rows=True)
    rs = m.train_rows_layout()[2]
    rng = np.random.default_rng(11)
    blocks = [
        _block(rng, [256], rs, d, 1),
        _block(rng, rng.permutation(np.arange(200, 257))[:50], rs, d, 64, bad_every=5, one_is_E=True),      # 13 x -1, 1 x E, 50 rows
        _block(rng, np.concatenate([[256, 0], rng.permutation(np.arange(190, 256))[:50]]), rs, d, 65, bad_every=5),      # 13 x -1, 52 rows
        _block(rng, rng.permutation(E), rs, d, E),
    ]
    wantE, wantb, union = np.zeros((E, d), F32), np.zeros(E, F32), set()
    m.profile(True)
    for j, (ids, vals) in enumerate(blocks):
        m.train_rows_import(torch.as_tensor(ids).cuda(), torch.as_tensor(vals).cuda(), first=j == 0)
        good = (ids >= 0) & (ids < E)
        wantE[ids[good]] = wantE[ids[good]] + vals[good, :d]      # float32 + float32, in call order
        wantb[ids[good]] = wantb[ids[good]] + vals[good, d]
        union |= set(ids[good].tolist())
        gE, gb = _table_grads(m, d)
        assert np.array_equal(gE, wantE) and np.array_equal(gb, wantb), j
        assert m.train_row_stats()["rows_last_step"] == len(union), j
        assert m.profile_read("train.rows.import")[1] == 1 and m.profile_read("train.rows.rezero")[1] == (1 if j == 0 else 0)
    assert len(union) == E
    # the pending union exports as it stands: every row once, the bits of the sum
    _, ids, vals, count = m.train_rows_export(False, ids=torch.empty(E, device="cuda:0", dtype=torch.int32), vals=torch.empty((E, rs), device="cuda:0"))
    ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    assert int(count.cpu()[0]) == E and np.array_equal(np.sort(ids), np.arange(E))
    assert np.array_equal(vals[:, :d], wantE[ids]) and np.array_equal(vals[:, d], wantb[ids])
    assert m.profile_read("train.rows.export")[1] == 1
    # a second `first`: the lot is gone
    ids, vals = blocks[0]
    m.train_rows_import(torch.as_tensor(ids).cuda(), torch.as_tensor(vals).cuda(), first=True)
    gE, gb = _table_grads(m, d)
    assert m.train_row_stats()["rows_last_step"] == 1
    assert np.array_equal(gE[256], vals[0, :d]) and gb[256] == vals[0, d] and not gE[:256].any() and not gb[:256].any()
    # first == 0 with nothing pending (an update consumed it) is refused
    m.train_rows_apply(torch.zeros(m.train_rows_layout()[1], device="cuda:0"))
    with pytest.raises(CoperError) as e:
        m.train_rows_import(torch.as_tensor(ids).cuda(), torch.as_tensor(vals).cuda(), first=False)
    assert e.value.code == 5
    m.close()


# ------------------------------------------------------------------------------------------------ S.3
@pytest.mark.parametrize("N", [1, 9])
def test_imported_rows_are_caught_up(N):
    """The planted-slot set-up of G.1 (tests/test_gpu_train_rows.py): rows 128 .. 256 get no gradient for N steps.  Then every second of
    them reaches the handle ONLY through an import (zero values) and update N + 1 runs as coper_train_rows_apply on a zero small vector
    -- a zero-gradient update of every leaf; the other rows are left to the final sync.  Against the float64 loop of N + 1 dense
    zero-gradient updates the deferred deviation may not exceed the larger of the dense twin's (N steps + coper_train_apply on a zero
    flat vector) and 4 float32 ulps of the largest compared magnitude: G.1's bound.  A row the import had not brought current would have
    missed N updates."""
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
    models = {}
    for mode in ("deferred", "dense"):
        m = _model(md, p0, deferred_rows=mode == "deferred")
        m.load_optimizer_state(planted)
        models[mode] = m
    _, powers = models["dense"].optimizer_state()
    for step in range(N):
        batch = _batch_below(md, lo, B, L, seed=1000 + step)
        for m in models.values():
            m.train_step(batch)
    dm = models["deferred"]
    assert dm.train_row_stats()["max_gap"] == N
    rs, total = dm.train_rows_layout()[2], dm.train_rows_layout()[1]
    rows = np.arange(lo, E, 2, dtype=np.int32)          # 128, 130 .. 256
    dm.train_rows_import(torch.as_tensor(rows).cuda(), torch.zeros((rows.size, rs), device="cuda:0"), first=True)
    dm.train_rows_apply(torch.zeros(total, device="cuda:0"), 1.0)
    st = dm.train_row_stats()
    assert st["rows_last_step"] == rows.size and st["max_gap"] == N + 1      # (the odd rows: the sync's)
    models["dense"].train_apply(torch.zeros(models["dense"].train_grads_layout()[1], device="cuda:0"), 1.0)
    lr, b1, b2, eps = float(F32(md["learning_rate"])), float(F32(0.9)), float(F32(0.999)), float(F32(1e-8))
    want = {}
    for leaf in TABLES:
        p = np.asarray(p0[leaf], F32).astype(np.float64).reshape(planted[leaf][0].shape)[lo:]
        mm, vv, hh = (a[lo:].astype(np.float64) for a in planted[leaf])
        b1p, b2p = powers["beta1_power"], powers["beta2_power"]
        for _ in range(N + 1):
            lr_t = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
            mm, vv = b1 * mm, b2 * vv
            hh = np.maximum(hh, vv)
            p = p - lr_t * mm / (np.sqrt(hh) + eps)
            b1p, b2p = b1p * b1, b2p * b2
        want.update({(leaf, "p"): p, (leaf, "m"): mm, (leaf, "v"): vv, (leaf, "vh"): hh})
    got = {mode: _state(m) for mode, m in models.items()}
    assert dm.train_row_stats()["rows_behind"] == 0
    for sel, what in ((slice(0, None, 2), "imported"), (slice(1, None, 2), "synced")):
        for key, w in want.items():
            dev = {mode: float(np.abs(got[mode][key].reshape((E,) + w.shape[1:])[lo:][sel] - w[sel]).max()) for mode in got}
            ulp4 = 4.0 * float(np.spacing(F32(np.abs(w[sel]).max())))
            print("S.3 N=%d %s %s/%s: deferred %.3e dense %.3e (4 ulp %.3e)" % (N, what, key[0], key[1], dev["deferred"], dev["dense"], ulp4))
            assert dev["deferred"] <= max(dev["dense"], ulp4), (N, what, key, dev, ulp4)
    for m in models.values():
        m.close()


# ------------------------------------------------------------------------------------------------ S.4
UPDATES = 3


@functools.lru_cache(maxsize=None)
def _trajectory(name, micro, clip=S.CLIP):
    """The float64 oracle over UPDATES updates of `micro` gap batches each, clipping at `clip` (computed once per model, micro-batch
    count and clip) -> ([(mean loss, mean gradients, their norm)] per update, the final state)."""
    md = _md(name)
    ref, opt = S.new_oracle(md, _p0(md), clip)
    out = []
    for u in range(UPDATES):
        losses, grads = [], []
        for i in range(micro):
            lo, g = S.oracle_backward(ref, md, _gap_batch(md, u * micro + i), SEED, u * micro + i)
            losses.append(lo)
            grads.append(g)
        mean, gn = S.oracle_update(ref, opt, grads)
        out.append((float(np.mean(losses)), mean, gn))
    return out, {k: np.array(v) for k, v in ref.items()}, _oracle_state(ref, opt)


def _small_slices(small, layout, scale=1.0):
    a = small.cpu().numpy() * F32(scale)
    return {leaf: a[off:off + n] for leaf, (off, n) in layout.items()}


def _route_update(m, route, md, u):
    """One update by `route` -> (mean loss, {leaf: mean gradient as the update applied it})"""
    leaves = m.trainable_leaves()
    if route in ("dense", "rows"):
        b = _gap_batch(md, u)
        loss = float((m.train_backward(b) if route == "dense" else m.train_rows_backward(b)).cpu()[0])
        grads = {leaf: _grad(m, leaf) for leaf in leaves}
        m.train_apply() if route == "dense" else m.train_rows_apply(None, 1.0)
        return loss, grads
    if route == "dense_m2":
        flat, loss = None, 0.0
        for i in range(2):
            loss += 0.5 * float(m.train_backward(_gap_batch(md, 2 * u + i)).cpu()[0])
            flat = m.train_grads_export(flat, accumulate=i > 0)
        grads = S.flat_slices(flat.cpu().numpy() * F32(0.5), m.train_grads_layout()[0])
        m.train_apply(flat, 0.5)
        return loss, grads
    layout = m.train_rows_layout()[0]
    micro = 2 if route == "rows_m2" else 1
    small, blocks, loss = None, [], 0.0
    for i in range(micro):
        loss += float(m.train_rows_backward(_gap_batch(md, micro * u + i)).cpu()[0]) / micro
        small, ids, vals, _ = m.train_rows_export(small, accumulate=i > 0)
        blocks.append((ids, vals))
    for i, (ids, vals) in enumerate(blocks):
        m.train_rows_import(ids, vals, first=i == 0)
    grads = _small_slices(small, layout, 1.0 / micro)
    for leaf in TABLES:
        grads[leaf] = _grad(m, leaf) * F32(1.0 / micro)
    m.train_rows_apply(small, 1.0 / micro)
    return loss, grads


@pytest.mark.parametrize("name,clip", [pytest.param("cpg_linear", S.CLIP, id="cpg_linear"), pytest.param("plain", S.CLIP, id="plain"),
                                       pytest.param("cpg_linear", 0.1, id="cpg_linear-clip0.1")])
def test_the_routes_agree_with_the_oracle(name, clip):
    """Three free-running updates on the gap batches of G.2, dropout on: rows_backward + rows_apply(NULL, 1); rows_backward + export +
    import(first) + rows_apply(small, 1); two micro-batches accumulated and applied with scale 0.5 -- each against the float64 oracle of
    the same updates (split_common.oracle_backward / oracle_update: the mean of the micro-batch gradients through one AMSGrad.step), with
    a dense twin (mode off: train_backward + train_apply, and its two-micro-batch form) beside them, held to the same bounds.  Per
    update: the loss by the non-tight law, the gradients by check_grads (2e-4 by _rel_err), the norm to 1e-4.  After the last update and
    a train_sync_rows(): every variable by check_variables, whose gradient term takes the sum of the three updates' gradient deviations
    (each update moves a variable by its own deviation's worth, and they add), and every slot of every row by G.2's law: within twice
    the dense twin's deviation plus the absolute floor.
    clip0.1: the same with clip_norm = 0.1 on every side, below half the oracle's global norm in every update (asserted) -- at 5.0 the
    clip factor is 1 whatever k_rows_sumsq adds, and so is |scale| sqrt(ss) of k_rows_update under the micro-batch route's scale 0.5.
    There the slots are held WITHOUT the absolute floor, dev <= 2 dev_twin + 1e-4 max|w| (the law of
    tests/test_gpu_train_rows_edges.py): v is around 1e-9 and m around 1e-4, and the first AMSGrad updates move p by lr_t sign(g)
    whatever the scale, so a wrong clip factor shows in the slots or nowhere."""
    md = _md(name)
    p0 = _p0(md)
    final = {}
    for route, micro in (("dense", 1), ("rows", 1), ("rows_block", 1), ("dense_m2", 2), ("rows_m2", 2)):
        traj, ref, want_state = _trajectory(name, micro, clip)
        m = _model(md, p0, deferred_rows=route.startswith("rows"), clip_norm=clip)
        dg_sum = {}
        for u in range(UPDATES):
            loss_o, mean_o, gn_o = traj[u]
            if clip != S.CLIP:
                assert gn_o > 2.0 * clip, (micro, u, gn_o)
            loss, grads = _route_update(m, route, md, u)
            _loss_close(loss, loss_o)
            dg = S.check_grads(grads, mean_o, gn_o, "%s update %d" % (route, u))
            for k, v in dg.items():
                dg_sum[k] = dg_sum.get(k, 0.0) + v
            gn = m.train_grad("ent_emb")[1]
            assert abs(gn - gn_o) < 1e-4 * gn_o, (route, u, gn, gn_o)
        if route.startswith("rows"):
            assert m.train_row_stats()["rows_behind"] > 0      # (gaps: the rows only some updates named)
        got = _state(m)
        S.check_variables(md, {k: got[(k, "p")] for k in ref}, ref, dg_sum, route)
        final[route] = (got, want_state)
        m.close()
    for route, twin in (("rows", "dense"), ("rows_block", "dense"), ("rows_m2", "dense_m2")):
        got, want_state = final[route]
        for key, w in sorted(want_state.items()):
            if key[1] == "p":
                continue
            dev = float(np.abs(got[key].reshape(w.shape) - w).max())
            dev_twin = float(np.abs(final[twin][0][key].reshape(w.shape) - w).max())
            floor = 2e-5 + 1e-5 * float(np.abs(w).max()) if clip == S.CLIP else 1e-4 * float(np.abs(w).max())
            print("S.4 %s clip %g %s %s/%s: %.3e dense %.3e floor %.3e" % (name, clip, route, key[0], key[1], dev, dev_twin, floor))
            assert dev <= 2.0 * dev_twin + floor, (route, key, dev, dev_twin, floor)


# ------------------------------------------------------------------------------------------------ S.5
def test_state_rules():
    lib = _lib.load()
    md = _md("cpg_linear")
    p0 = _p0(md)
    _model(md, p0).close()      # (whatever the process allocates once is there before the ledger is read)
    live0 = lib.coper_live_device_bytes()
    ref, opt = S.new_oracle(md, p0)
    m = _model(md, p0, deferred_rows=True)
    total = m.train_rows_layout()[1]
    b0, b1 = _gap_batch(md, 0), _gap_batch(md, 1)
    # nothing pending
    for call in (lambda: m.train_rows_apply(), lambda: m.train_rows_export()):
        with pytest.raises(CoperError) as e:
            call()
        assert e.value.code == 5
    # 1-vs-all: refused, the handle stays usable
    dense_labels = np.zeros((B, E), F32)
    dense_labels[np.arange(B), b0["lookup_values"][:, 0]] = 1.0
    with pytest.raises(CoperError, match="deferred-rows mode") as e:
        m.train_rows_backward(dict(e1=b0["e1"], rel=b0["rel"], e2_multi=dense_labels))
    assert e.value.code == 7
    with pytest.raises(CoperError) as e:
        m.train_rows_backward(dict(e1=b0["e1"], rel=b0["rel"], lab_indptr=np.arange(B + 1, dtype=np.int64), lab_idx=np.zeros(B, np.int64)))
    assert e.value.code == 7
    # a refused call clears nothing: backward, a refused export and a refused apply, then the apply
    loss_o, g0 = S.oracle_backward(ref, md, b0, SEED, 0)
    S.oracle_update(ref, opt, [g0])
    _loss_close(float(m.train_rows_backward(b0).cpu()[0]), loss_o)
    with pytest.raises(CoperError) as e:
        m.train_rows_apply(torch.zeros(total - 64, device="cuda:0"))
    assert e.value.code == 1
    with pytest.raises(CoperError) as e:
        m.train_rows_apply(None, float("nan"))
    assert e.value.code == 1
    with pytest.raises(CoperError, match="deferred-rows mode") as e:
        m.train_apply()
    assert e.value.code == 7
    m.train_rows_apply()
    # a train_step between backward and apply clears pending; the step itself is where the oracle puts it
    m.train_rows_backward(b1)           # (dropout counter 1; its gradient is dropped)
    ob = dict(ref)
    S.oracle_backward(ob, md, b1, SEED, 1)
    for k in ref:                       # (the dropped backward moved the moving statistics)
        if k.endswith(("moving_mean", "moving_variance")):
            ref[k] = ob[k]
    from tests.test_gpu_train_rows import _oracle_step
    _loss_close(float(m.train_step(b1).cpu()[0]), _oracle_step(md, ref, opt, b1, 2))
    with pytest.raises(CoperError) as e:
        m.train_rows_apply()
    assert e.value.code == 5
    # ... and so does a forward
    m.train_rows_backward(b0)
    m.train_forward(b0)
    with pytest.raises(CoperError) as e:
        m.train_rows_apply()
    assert e.value.code == 5
    # ... and a mode switch
    m.train_rows_backward(b0)
    m.train_defer_rows(False)
    for call in (lambda: m.train_rows_backward(b0), lambda: m.train_rows_export(), lambda: m.train_rows_apply(),
                 lambda: m.train_rows_import(torch.zeros(1, device="cuda:0", dtype=torch.int32), torch.zeros((1, 44), device="cuda:0"), first=True)):
        with pytest.raises(CoperError) as e:      # the new calls with the mode off
            call()
        assert e.value.code == 5
    assert m.train_rows_layout()[1] == total
    m.train_defer_rows(True)
    with pytest.raises(CoperError) as e:
        m.train_rows_apply()
    assert e.value.code == 5
    m.close()
    assert lib.coper_live_device_bytes() == live0


def test_prepare_between_backward_and_apply_changes_nothing():
    """Handle A: rows_backward, export (kept), an evaluation pass (rank_pass: prepare() syncs the rows and folds BN), rows_apply(NULL).
    Handle B, from the same variables, never evaluates: import(first) of A's block, rows_apply of A's small vector.  Both updates read
    the same gradient bits (the export is a copy, 0 + g = g), and with the clip out of reach the element factor is exactly 1 whatever
    order the norm was summed in: every trainable variable and every slot of A equals B's bit for bit."""
    lib = _lib.load()
    md = _md("cpg_linear")
    p0 = _p0(md)
    _model(md, p0).close()
    live0 = lib.coper_live_device_bytes()
    a, b =(_model(md, p0, deferred_rows=True, clip_norm=1e30) for _ in range(2))
    batch = _gap_batch(md, 0)
    a.train_rows_backward(batch)
    small, ids, vals, count = a.train_rows_export()
    q = cdata.synthetic_queries(md, 12, seed=3)
    ranks, _ = a.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
    assert ranks.numel() == 12
    a.train_rows_apply()
    b.train_rows_import(ids, vals, first=True)
    assert b.train_row_stats()["rows_last_step"] == int(count.cpu()[0]) == _ids(batch).size
    b.train_rows_apply(small, 1.0)
    sa, sb = _state(a), _state(b)
    for key in sorted(sa):
        if key[0].endswith(("moving_mean", "moving_variance")):      # (A's backward moved them; B ran none)
            continue
        assert _same_bits(sa[key], sb[key]), key
    changed = sum(not _same_bits(sa[(k, "p")], np.asarray(p0[k], F32).reshape(sa[(k, "p")].shape)) for k in a.trainable_leaves())
    assert changed > 0      # (the update was one)
    a.close()
    b.close()
    assert lib.coper_live_device_bytes() == live0
