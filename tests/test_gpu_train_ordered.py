"""GPU tests of ordered rows (include/coper_hip.h "Ordered rows"): the switch on a deterministic training state that builds
the sampled scorer's table gradient from a stable sort of the batch's ids, one writer per row -- bit-reproducible sampled steps at any
number of entities, deferred rows on a deterministic state, row blocks in ascending id, byte-identical replicas.

Shapes, batches and the bit comparison come from tests/test_gpu_train_deterministic.py (D) and tests/test_gpu_train_rows.py (R); the
oracle bounds are D.test_deterministic_step_matches_oracle's (loss 2e-5, gradients 2e-4 of the largest entry with a floor of 1e-3 of
the norm, norm 1e-4) and R's G.2 law for trajectories with gaps.  The sort tile is read from the header, so the edge cases sit on it."""
import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from coper_amd import parallel
from tests import test_gpu_train_deterministic as D
from tests import test_gpu_train_rows as R
from tests.test_train_order_abi import kernel_constants

pytestmark = pytest.mark.gpu

SEED = D._SEED
F32 = np.float32
TILE = kernel_constants()["COPER_ORDER_SORT_TILE"]
EINVAL, ESTATE, EUNSUPPORTED = 1, 5, 7
ORDER_NAMES = ("train.order.sort", "train.order.heads", "train.order.reduce", "train.order.sumsq")


def _model(md, p0, ordered=True, deferred=False, deterministic=True):
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, F32)) for k, v in p0.items()})
    m.train_init(seed=SEED, deterministic=deterministic, ordered_rows=ordered, deferred_rows=deferred)
    assert m.train_rows_ordered == (1 if ordered else 0) and m.train_rows_deferred == (1 if deferred else 0)
    return m


def _p0(md):
    return cdata.synthetic_params(md, seed=21, ent_std=0.1)


def _small_md(E, d=12, h=3, w=4):
    """The narrow model of D.test_flag_and_refusals (d = 12, three channels, 2 x 2 filters) at E entities."""
    return dict(D._md("cpg_linear"), num_ent=E, ent_emb_size=d, emb_h=h, emb_w=w, conv_num_channels=3, conv_filter_height=2, conv_filter_width=2)


def _outs(m, loss):
    """D._outputs behind a sync (deferred rows: the raw tables are current only then), and the row words' statistics."""
    m.train_sync_rows()
    out = D._outputs(m, loss)
    for k, v in m.train_row_stats().items():
        out["rows/" + k] = np.int64(v)
    return out


def _save(m):
    m.train_sync_rows()
    return {k: v.clone() for k, v in m._tensors.items()}, m.optimizer_state()


def _restore(m, saved):
    m.load_parameters({k: v.clone() for k, v in saved[0].items()})
    m.load_optimizer_state(*saved[1])


def _clamped(batch, E):
    """The batch as the step's kernels read it: ids outside [0, E) are row 0 (what the oracle, which indexes, has to be given)."""
    out = dict(batch)
    for k in ("e1", "lookup_values"):
        a = np.array(batch[k])
        a[(a < 0) | (a >= E)] = 0
        out[k] = a
    return out


def _check_oracle(m, md, p0, batch, zero_rows_outside=None):
    """One step of `m` from p0 against the float64 oracle, within D.test_deterministic_step_matches_oracle's bounds."""
    from oracle import coper_train_oracle as T
    ref = {k: np.array(v, np.float64) for k, v in p0.items()}
    opt = T.AMSGrad(T.trainable_names(md), ref, lr=md["learning_rate"], clip=5.0)
    cb = _clamped(batch, md["num_ent"])
    ob = dict(e1=cb["e1"], rel=cb["rel"], lookup=cb["lookup_values"], labels=cb["e2_multi"])
    loss_o, grads_o, gn_o = T.train_step(ref, md, ob, opt, seed=SEED, step=0, momentum=md["batch_norm_momentum"])
    loss = float(m.train_step(batch).cpu()[0])
    print("loss %.9g oracle %.9g" % (loss, loss_o))
    assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (loss, loss_o)
    for leaf in T.trainable_names(md):
        g, gn = m.train_grad(leaf)
        g = g.cpu().numpy().reshape(grads_o[leaf].shape)
        err = D._rel_err(g, grads_o[leaf], 1e-3 * gn_o)
        print("  %-40s rel err %.3g" % (leaf, err))
        assert err < 2e-4, (leaf, err)
        if zero_rows_outside is not None and leaf in ("ent_emb", "pred_bias"):
            mask = np.ones(md["num_ent"], bool)
            mask[zero_rows_outside] = False
            assert not g[mask].any(), leaf      # every row the batch does not name is exactly zero
            assert np.abs(g[~mask]).max() > 0
    print("  norm %.9g oracle %.9g" % (gn, gn_o))
    assert abs(gn - gn_o) < 1e-4 * gn_o


# ------------------------------------------------------------------------------------------------ 1
def test_switch_and_refusals():
    from coper_amd._lib import CoperError
    from coper_amd.models import ConvE
    md = D._md("cpg_linear")
    p0 = _p0(md)
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, F32)) for k, v in p0.items()})
    assert m._lib.coper_train_rows_ordered(m._h) == -ESTATE
    assert m._lib.coper_train_order_rows(m._h, 1, None) == ESTATE      # before coper_train_init
    m.train_init(seed=SEED)                                            # a default-mode state
    with pytest.raises(CoperError, match="unordered") as e:
        m.train_order_rows(True)
    assert e.value.code == EUNSUPPORTED and m.train_rows_ordered == 0
    m.train_init(seed=SEED, deterministic=True)
    assert m.train_rows_ordered == 0
    with pytest.raises(CoperError, match="0 or 1") as e:
        m.train_order_rows(2)
    assert e.value.code == EINVAL
    # the switch OFF: the two pinned refusals, with their texts
    with pytest.raises(CoperError, match="the unique-row list and the atomic scorer backward are unordered") as e:
        m.train_defer_rows(True)
    assert e.value.code == EUNSUPPORTED and m.train_rows_deferred == 0
    m.train_order_rows(True)
    assert m.train_rows_ordered == 1
    m.train_order_rows(True)      # (idempotent)
    m.train_defer_rows(True)
    assert m.train_rows_deferred == 1
    with pytest.raises(CoperError, match="disable deferred rows first") as e:
        m.train_order_rows(False)
    assert e.value.code == ESTATE and m.train_rows_ordered == 1
    with pytest.raises(CoperError) as e:
        m.train_defer_rows(2)
    assert e.value.code == EINVAL
    m.train_defer_rows(False)
    m.train_order_rows(False)
    assert m.train_rows_ordered == 0
    # switching clears what a split step left pending
    m.train_backward(D._batch(md, "sampled", 8, 5, seed=1))
    m.train_order_rows(True)
    with pytest.raises(CoperError, match="no gradients pending") as e:
        m.train_apply()
    assert e.value.code == ESTATE
    # train_init resets the switch
    m.train_init(seed=SEED, deterministic=True)
    assert m.train_rows_ordered == 0 and m.train_rows_deferred == 0
    m.train_init(seed=SEED, deterministic=True, ordered_rows=True, deferred_rows=True)
    assert m.train_rows_ordered == 1 and m.train_rows_deferred == 1
    m.close()
    # the switch OFF: the 512 MiB refusal of the deterministic mode (test_past_the_cap has the same handle with the switch on)
    md = _small_md(1048583)
    m = _model(md, _p0(md), ordered=False)
    with pytest.raises(CoperError, match="512 MiB") as e:
        m.train_step(D._batch(md, "sampled", 129, 5, seed=1))
    assert e.value.code == EUNSUPPORTED and "take the atomic scorer backward" in str(e.value)
    m.close()


# ------------------------------------------------------------------------------------------------ 2
def test_past_the_cap():
    """num_ent = 1048583, d = 12, B = 129, L = 5: B * num_ent * 4 > 512 MiB.  Refused with the switch off (test_switch_and_refusals);
    with it on one step has the same bits on two handles and again from the restored state, the named rows of d(ent_emb) /
    d(pred_bias) follow the float64 oracle and every other row is exactly zero."""
    md = _small_md(1048583)
    B, L = 129, 5
    assert B * md["num_ent"] * 4 > 512 * 1024 * 1024
    p0 = _p0(md)
    batch = D._batch(md, "sampled", B, L, seed=1)
    a, b = _model(md, p0), _model(md, p0)
    saved = _save(a)
    fa, fb = a.train_forward(batch, want_predictions=True, want_h=True), b.train_forward(batch, want_predictions=True, want_h=True)
    for x, y in zip(fa, fb):
        assert torch.equal(x, y)
    oa, ob = _outs(a, a.train_step(batch)), _outs(b, b.train_step(batch))
    D._assert_same_bits(oa, ob, "two handles")
    _restore(a, saved)
    D._assert_same_bits(_outs(a, a.train_step(batch)), oa, "from the restored state")
    b.close()
    _restore(a, saved)
    named = np.unique(np.concatenate([batch["e1"].reshape(-1), batch["lookup_values"].reshape(-1).astype(np.int64)]))
    _check_oracle(a, md, p0, batch, zero_rows_outside=named)
    a.close()


# ------------------------------------------------------------------------------------------------ 3
def _bits_case(name, B, L=37, deferred=False, history=False, md=None, batch_fn=None, steps=3, repeats=5):
    """D._bits_case's protocol with the switch on: forward x 3, `steps` steps on two handles, `repeats` repeats from a restored state.
    history: handle B first runs a B = 300, L = 64 batch (its row lists and workspaces grow past what the case needs) and is put back."""
    md = md or D._md(name)
    p0 = _p0(md)
    make = batch_fn or (lambda seed: D._batch(md, "sampled", B, L, seed))
    a, b = _model(md, p0, deferred=deferred), _model(md, p0, deferred=deferred)
    if history:
        start = _save(b)
        b.train_step(D._batch(md, "sampled", 300, 64, 77))
        _restore(b, start)
    batch = make(400)
    fa = a.train_forward(batch, want_predictions=True, want_h=True)
    fb = b.train_forward(batch, want_predictions=True, want_h=True)
    fa2 = a.train_forward(batch, want_predictions=True, want_h=True)
    for x, y, z in zip(fa, fb, fa2):
        assert torch.equal(x, y) and torch.equal(x, z)
    for step in range(steps):
        batch = make(400 + step)
        if step == steps - 1:
            saved = _save(a)
        oa = _outs(a, a.train_step(batch))
        ob = _outs(b, b.train_step(batch))
        D._assert_same_bits(oa, ob, "step %d, two handles" % step)
        if step == 0:
            assert np.array_equal(oa["loss"], fa[0].cpu().numpy())      # (the forward drew this step's masks)
    for rep in range(repeats):
        _restore(a, saved)
        D._assert_same_bits(_outs(a, a.train_step(batch)), oa, "repeat %d from the restored state" % rep)
    a.close()
    b.close()


@pytest.mark.parametrize("deferred", [False, True], ids=["ordered", "ordered_deferred"])
@pytest.mark.parametrize("B", [1, 77, 300])
@pytest.mark.parametrize("name", ["cpg_linear", "cpg_mlp_bn", "plain", "lookup", "cpg_linear_concat"])
def test_bits_across_handles_and_repeats(name, B, deferred):
    _bits_case(name, B, deferred=deferred)


@pytest.mark.parametrize("deferred", [False, True], ids=["ordered", "ordered_deferred"])
def test_bits_across_histories(deferred):
    """Handle B's row-list capacity, sort workspace and slab grew from a B = 300, L = 64 batch before it was put back to the state."""
    _bits_case("cpg_linear", 77, deferred=deferred, history=True)


def test_bits_on_a_side_stream():
    side = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _bits_case("cpg_linear", 77, deferred=True)
    side.synchronize()


# ------------------------------------------------------------------------------------------------ 4
def _shape_with_entries(n):
    """(B, L) with B (L + 1) == n sorted entries (the lookup ids and the e1 ids), 2 <= B <= 64."""
    for b in range(64, 1, -1):
        if n % b == 0 and n // b >= 2:
            return b, n // b - 1
    raise AssertionError(n)


def _edge_batches():
    big = D._md("cpg_linear")
    E = big["num_ent"]
    cases = {}

    def sampled(md, B, L, seed=31, **kw):
        return md, D._batch(md, "sampled", B, L, seed, **kw)
    cases["L1"] = sampled(big, 77, 1)
    for tag, n in (("tile_minus_1", TILE - 1), ("tile", TILE), ("tile_plus_1", TILE + 1)):
        cases["entries_" + tag] = sampled(big, *_shape_with_entries(n))
    for tag, n in (("tile_minus_1", TILE - 1), ("tile", TILE), ("tile_plus_1", TILE + 1)):      # B L itself on the tile
        b_, l1 = _shape_with_entries(n)
        cases["BL_" + tag] = sampled(big, b_, l1 + 1)
    cases["three_tiles"] = sampled(big, 77, (2 * TILE) // 77 + 8)         # more than two tiles
    for En in (211, 20011, 70001):                                        # one, two and three digit passes
        cases["E%d" % En] = sampled(_small_md(En), 33, 21)
    md, b = sampled(big, 40, 64)
    b["lookup_values"][:] = 7                                             # one segment of B L entries
    cases["hub"] = (md, b)
    cases["dup_in_row"] = sampled(big, 33, 9)                             # D._batch: an id at l = 0, 1 and L - 1 of every row
    md, b = sampled(big, 33, 9)
    b["lookup_values"][0, 0], b["lookup_values"][1, 2], b["lookup_values"][2, 3] = -1, E, 0
    b["lookup_values"][5, 4] = E + 9
    b["e1"][3], b["e1"][4] = E, -2
    cases["clamped_ids"] = (md, b)
    md, b = sampled(big, 33, 9)
    b["lookup_values"][:, 5] = E - 1
    b["e1"][7] = E - 1
    cases["last_id"] = (md, b)
    cases["one_e1"] = sampled(big, 77, 9, one_e1=True)
    cases["d10"] = sampled(_small_md(211, d=10, h=5, w=2), 33, 9)         # d % 4 != 0: the scalar route
    return cases


_EDGES = _edge_batches()


@pytest.mark.parametrize("case", sorted(_EDGES))
def test_sort_and_segment_edges(case):
    md, batch = _EDGES[case]
    p0 = _p0(md)
    for deferred in (False, True):
        a, b = _model(md, p0, deferred=deferred), _model(md, p0, deferred=deferred)
        start = _save(a)
        oa, ob = _outs(a, a.train_step(batch)), _outs(b, b.train_step(batch))
        D._assert_same_bits(oa, ob, "%s deferred=%d" % (case, deferred))
        _restore(a, start)
        D._assert_same_bits(_outs(a, a.train_step(batch)), oa, "%s deferred=%d, restored" % (case, deferred))
        a.close()
        b.close()
        m = _model(md, p0, deferred=deferred)
        _check_oracle(m, md, p0, batch)
        m.close()


# ------------------------------------------------------------------------------------------------ 5
def test_the_list_is_the_stable_sorts():
    md = R._md("cpg_linear")
    E, d = md["num_ent"], md["ent_emb_size"]
    m = _model(md, _p0(md), deferred=True)
    batch = R._batch_below(md, E, 16, 24, seed=7)
    batch["lookup_values"][0, 0], batch["lookup_values"][1, 1], batch["e1"][2] = E + 5, -3, E
    m.train_rows_backward(batch)
    _, ids, vals, count = m.train_rows_export()
    n = int(count.cpu()[0])
    ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    want = R._ids(batch)
    assert n == want.size and np.array_equal(ids[:n], want) and (ids[n:] == -1).all()
    dE, db = m.train_grad("ent_emb")[0].cpu().numpy().reshape(E, d), m.train_grad("pred_bias")[0].cpu().numpy()
    assert vals[:n, :d].tobytes() == dE[want].tobytes() and vals[:n, d].tobytes() == db[want].tobytes() and not vals[:n, d + 1:].any()
    mask = np.ones(E, bool)
    mask[want] = False
    assert not dE[mask].any() and not db[mask].any()
    # two overlapping blocks in shuffled id order: the pending list is ascending again, the rows are the blocks' sums in call order
    rng = np.random.default_rng(3)
    perm = rng.permutation(n)
    blocks = [perm[:2 * n // 3], perm[n // 3:]]
    for i, sel in enumerate(blocks):
        m.train_rows_import(torch.as_tensor(ids[sel].copy()).cuda(), torch.as_tensor(vals[sel].copy()).cuda(), first=i == 0)
    _, ids2, vals2, count2 = m.train_rows_export(small=False)
    n2 = int(count2.cpu()[0])
    ids2, vals2 = ids2.cpu().numpy(), vals2.cpu().numpy()
    assert n2 == n and np.array_equal(ids2[:n2], want) and (ids2[n2:] == -1).all()
    times = np.zeros(n, F32)
    for sel in blocks:
        times[sel] += 1
    assert set(times) == {1.0, 2.0}
    assert vals2[:n].tobytes() == (vals[:n] * times[:, None]).astype(F32).tobytes()      # (g, or g + g)
    m.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("pair", ["dense_S", "deferred"])
def test_ordered_against_the_routes_it_replaces(pair):
    """From one state and one batch: ordered vs deterministic = 1 (the dense S route) at E = 211; ordered + deferred vs default deferred
    rows.  Loss, every gradient and the norm within the oracle bounds -- not to the bit."""
    md = D._md("cpg_mlp_bn")
    p0 = _p0(md)
    if pair == "dense_S":
        a, b = _model(md, p0, ordered=False), _model(md, p0)
    else:
        a, b = _model(md, p0, ordered=False, deferred=True, deterministic=False), _model(md, p0, deferred=True)
    batch = D._batch(md, "sampled", 77, 37, seed=900)
    la, lb = float(a.train_step(batch).cpu()[0]), float(b.train_step(batch).cpu()[0])
    assert abs(la - lb) < 2e-5 * max(1.0, abs(la)), (la, lb)
    gn = a.train_grad("ent_emb")[1]
    for leaf in a.trainable_leaves():
        (ga, na), (gb, nb) = a.train_grad(leaf), b.train_grad(leaf)
        assert D._rel_err(gb.cpu().numpy(), ga.cpu().numpy(), 1e-3 * gn) < 2e-4, leaf
        assert abs(na - nb) < 1e-4 * na
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 7
SD = np.arange(120, 160)      # named in step 2 alone: one update behind after step 3 (SC: two, SB: three, the rest: four)


def _gap_batch(md, step):
    batch = R._gap_batch(md, step)
    if step == 2:
        batch["lookup_values"][:, 7] = np.random.default_rng(50).choice(SD, R.B)
    return batch


def test_gaps_in_ordered_deferred_mode():
    md = R._md("cpg_linear")
    p0 = _p0(md)
    ref, opt = R._oracle(md, p0)
    models = {"deferred": _model(md, p0, deferred=True), "dense": _model(md, p0)}
    for step in range(4):
        batch = _gap_batch(md, step)
        loss_o = R._oracle_step(md, ref, opt, batch, step)
        for m in models.values():
            R._loss_close(float(m.train_step(batch).cpu()[0]), loss_o)
    st = models["deferred"].train_row_stats()
    assert st["rows_behind"] > 0 and st["max_gap"] == 4, st
    got = {mode: R._state(m) for mode, m in models.items()}
    want = R._oracle_state(ref, opt)
    for key, w in sorted(want.items()):
        dev = {mode: float(np.abs(got[mode][key].reshape(w.shape) - w).max()) for mode in got}
        floor = 2e-5 + 1e-5 * float(np.abs(w).max())
        print("%s/%s: deferred %.3e dense %.3e floor %.3e" % (key[0], key[1], dev["deferred"], dev["dense"], floor))
        assert dev["deferred"] <= 2.0 * dev["dense"] + floor, (key, dev, floor)
    # the same sequence on a fresh handle: the same bits in every variable, slot and row word
    again = _model(md, p0, deferred=True)
    for step in range(4):
        again.train_step(_gap_batch(md, step))
    assert again.train_row_stats() == st
    second = R._state(again)
    assert again.train_row_stats() == models["deferred"].train_row_stats()
    assert sorted(second) == sorted(got["deferred"])
    for key in second:
        assert second[key].tobytes() == got["deferred"][key].tobytes(), key
    for m in list(models.values()) + [again]:
        m.close()


# ------------------------------------------------------------------------------------------------ 8
def _full_state(m):
    out = {"%s/%s" % k: v for k, v in R._state(m).items()}
    _, powers = m.optimizer_state()
    for k, v in powers.items():
        out["power/" + k] = np.float64(v)
    for k, v in m.train_row_stats().items():
        out["rows/" + k] = np.int64(v)
    return out


def _replica_pair(md, p0, updates=2):
    ranks = [_model(md, p0, deferred=True) for _ in range(2)]
    for u in range(updates):
        batch = R._batch_below(md, md["num_ent"], 16, 12, seed=600 + u)
        exported = []
        for r, m in enumerate(ranks):
            m.train_rows_backward(parallel.shard_batch(batch, r, 2))
            exported.append(m.train_rows_export())
        for r in range(2):      # a block is ascending and closed by -1s
            ids, n = exported[r][1].cpu().numpy(), int(exported[r][3].cpu()[0])
            assert (np.diff(ids[:n]) > 0).all() and (ids[n:] == -1).all()
        small = exported[0][0] + exported[1][0]      # the all-reduce
        for m in ranks:
            for r in range(2):
                m.train_rows_import(exported[r][1], exported[r][2], first=r == 0)
            m.train_rows_apply(small, 0.5)
    states = [_full_state(m) for m in ranks]
    for m in ranks:
        m.close()
    return states


def test_replicas_in_one_process_are_byte_identical():
    md = R._md("cpg_linear")
    p0 = _p0(md)
    s0, s1 = _replica_pair(md, p0)
    D._assert_same_bits(s0, s1, "rank 0 against rank 1")
    t0, t1 = _replica_pair(md, p0)
    D._assert_same_bits(s0, t0, "a second pair, rank 0")
    D._assert_same_bits(s1, t1, "a second pair, rank 1")

    # two micro-batches of accumulation on one handle reproduce their own bits on a fresh handle
    def accumulate():
        m = _model(md, p0, deferred=True)
        for u in range(2):
            small, blocks = None, []
            for i in range(2):
                m.train_rows_backward(R._batch_below(md, md["num_ent"], 8, 12, seed=700 + 2 * u + i))
                small, ids, vals, _ = m.train_rows_export(small=small, accumulate=True)
                blocks.append((ids, vals))
            for i, (ids, vals) in enumerate(blocks):
                m.train_rows_import(ids, vals, first=i == 0)
            m.train_rows_apply(small, 0.5)
        st = _full_state(m)
        m.close()
        return st
    D._assert_same_bits(accumulate(), accumulate(), "accumulation, a fresh handle")


# ------------------------------------------------------------------------------------------------ 9
def _order_counts(m):
    return {k: m.profile_read(k)[1] for k in ORDER_NAMES + ("train.rows.claim", "train.rows.sumsq")}


@pytest.mark.parametrize("E,passes", [(211, 1), (20011, 2)])
def test_route_proof(E, passes):
    md = _small_md(E)
    p0 = _p0(md)
    sampled = D._batch(md, "sampled", 33, 21, seed=5)
    m = _model(md, p0)
    start = _save(m)
    m.profile(True)
    _order_counts(m)
    m.train_step(sampled)
    assert _order_counts(m) == {"train.order.sort": 3 * passes, "train.order.heads": 2, "train.order.reduce": 1, "train.order.sumsq": 0,
                                "train.rows.claim": 0, "train.rows.sumsq": 0}
    m.train_forward(sampled)      # (deferred rows off: a forward needs no list)
    assert not any(_order_counts(m).values())
    # a 1-vs-all step on the same handle: none of the launches, and the bits of a plain deterministic = 1 handle
    plain = _model(md, p0, ordered=False)
    for route in ("csr", "dense"):
        _restore(m, start)
        _restore(plain, start)
        batch = D._batch(md, route, 33, 21, seed=6)
        om = D._outputs(m, m.train_step(batch))
        assert not any(_order_counts(m).values()), route
        D._assert_same_bits(om, D._outputs(plain, plain.train_step(batch)), "1-vs-all, " + route)
        if E > 211:
            break      # (one 1-vs-all route is enough at the larger table)
    plain.close()
    m.train_defer_rows(True)
    m.train_step(sampled)
    assert _order_counts(m) == {"train.order.sort": 3 * passes, "train.order.heads": 2, "train.order.reduce": 1, "train.order.sumsq": 1,
                                "train.rows.claim": 0, "train.rows.sumsq": 0}
    m.train_forward(sampled)      # (deferred rows: the forward's list is the sort's)
    c = _order_counts(m)
    assert c["train.order.sort"] == 3 * passes and c["train.order.heads"] == 2 and c["train.order.reduce"] == 0 and c["train.rows.claim"] == 0
    m.close()
