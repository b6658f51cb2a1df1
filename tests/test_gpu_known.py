"""The known-facts index on the GPU: coper_set_known_facts, coper_known_filter and the two fused entry points.

The expected CSR is always computed in NumPy from the HOST index (`_np_filter`); the expected answers are those of the existing
entry points (`predict_topk`, `rank_pass`) fed that NumPy CSR.  Every comparison is exact: ids as integers, values as bit
patterns, with the first differing query reported."""
import ctypes as C

import numpy as np
import pytest
import torch

from coper_amd import _lib
from coper_amd import data as cdata
from tests.helpers import known_filter_np as _np_filter

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, ESTATE = 1, 5


def _model(md, p, **kw):
    from coper_amd.models import ConvE
    return ConvE(md, device=DEV, **kw).load_parameters(p).prepare()


def _same_csr(got, want, what):
    gip, gix = (t.cpu().numpy() for t in got)
    wip, wix = want
    assert gip.dtype == np.int64 and gix.dtype == np.int64, what
    assert gip.shape == wip.shape, "%s: indptr of %s entries, want %s" % (what, gip.shape, wip.shape)
    bad = np.flatnonzero(gip != wip)
    assert bad.size == 0, "%s: indptr differs first at %d: got %d want %d" % (what, bad[0], gip[bad[0]], wip[bad[0]])
    assert gix.shape == wix.shape, what
    bad = np.flatnonzero(gix != wix)
    if bad.size:
        b = int(np.searchsorted(wip, bad[0], side="right") - 1)
        raise AssertionError("%s: %d of %d entries differ; first in query %d:\n got %s\nwant %s" % (
            what, bad.size, wix.size, b, gix[wip[b]:wip[b + 1]][:16].tolist(), wix[wip[b]:wip[b + 1]][:16].tolist()))


def _same(got, want, what):
    """Tuples of [B] or [B, k] tensors: ids equal, floats bit-equal; the first differing query is reported."""
    for g, w in zip(got, want):
        assert (g is None) == (w is None), what
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, what
        gb, wb = (g.view(torch.int32), w.view(torch.int32)) if g.dtype == torch.float32 else (g, w)
        bad = (gb != wb).reshape(g.shape[0], -1).any(dim=1)
        n_bad = int(bad.sum())
        if n_bad:
            b = int(torch.nonzero(bad)[0])
            raise AssertionError("%s: %d of %d queries differ; first %d:\n got %s\nwant %s" % (what, n_bad, g.shape[0], b, g[b].tolist(), w[b].tolist()))


def _answers_equal(m, kf, md, e1, rel, e2, what, k=10, rank=True):
    ip, ix = _np_filter(kf, md, e1, rel)
    _same_csr(m.known_filter(e1, rel), (ip, ix), what + " known_filter")
    _same(m.predict_topk_known(e1, rel, k), m.predict_topk(e1, rel, k, ip, ix), what + " predict_topk_known")
    if rank:
        _same(m.rank_pass_known(e1, rel, e2), m.rank_pass(e1, rel, e2, ip, ix), what + " rank_pass_known")
        _same(m.rank_pass_known(e1, rel, e2, want_equal=False), m.rank_pass(e1, rel, e2, ip, ix, want_equal=False), what + " rank_pass_known, ranks only")
    return ip, ix


# ---------------------------------------------------------------------------------------------------- 1. the smallest table
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_nations_lookup_edges(mode):
    md = cdata.model_descriptors("nations_cpg")
    E, R = md["num_ent"], md["num_rel"]
    q = cdata.synthetic_queries(md, 200, seed=2)
    kf = cdata.known_facts_from_queries(q)
    m = _model(md, cdata.synthetic_params(md, 3), score_mode=mode)
    assert m.set_known_facts(**kf) is m
    rng = np.random.default_rng(5)
    for B in (1, 63, 64, 65):
        e1, rel = q["e1"][:B].copy(), q["rel"][:B].copy()
        swap = rng.random(B) < 0.3                                   # some pairs drawn anew: present or absent as it falls
        e1[swap], rel[swap] = rng.integers(0, E, int(swap.sum())), rng.integers(0, R, int(swap.sum()))
        _answers_equal(m, kf, md, e1, rel, q["e2"][:B], "nations %s B=%d" % (mode, B), k=3)
    # every key absent: synthetic queries use the forward half of the relations only
    e1, rel = rng.integers(0, E, 70), np.full(70, R - 1, np.int64)
    ip, ix = m.known_filter(e1, rel)
    assert ip.tolist() == [0] * 71 and ix.numel() == 0
    _answers_equal(m, kf, md, e1, rel, q["e2"][:70], "nations %s all absent" % mode, k=3)
    # ids outside the model's range only have to stay in bounds: empty rows, the others right
    e1, rel = q["e1"][:10].copy(), q["rel"][:10].copy()
    e1[2], rel[5], e1[7] = E, R, -1
    ip, ix = _np_filter(kf, md, e1, rel)
    assert ip[3] == ip[2] and ip[6] == ip[5] and ip[8] == ip[7] and ip[-1] > 0
    _same_csr(m.known_filter(e1, rel), (ip, ix), "nations %s out-of-range ids" % mode)
    # B = 0
    ip, ix = m.known_filter(np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert ip.tolist() == [0] and ix.numel() == 0
    tv, ti = m.predict_topk_known(np.zeros(0, np.int64), np.zeros(0, np.int64), 3)
    assert tuple(tv.shape) == (0, 3) and tuple(ti.shape) == (0, 3)
    m.close()


# ---------------------------------------------------------------------------------------------------- 2. - 3. skewed rows at FB15k-237 shapes
LONG, LONG2 = (100, 5), (100, 6)          # the keys of the 3,000-tail and the 1,025-tail row


@pytest.fixture(scope="module")
def fb():
    md = cdata.model_descriptors("fb15k237_cpg")
    return md, cdata.synthetic_params(md, 0), _skewed_index(md)


def _skewed_index(md):
    """One row of 3,000 tails, one of 1,025, a run of 1,500 single-tail rows, and the first and the last possible key."""
    E, R = int(md["num_ent"]), int(md["num_rel"])
    rng = np.random.default_rng(17)
    rows = {(0, 0): np.array([7], np.int64), (E - 1, R - 1): np.array([0, E - 1], np.int64),
            LONG: np.sort(rng.choice(E, 3000, replace=False)).astype(np.int64),
            LONG2: np.sort(rng.choice(E, 1025, replace=False)).astype(np.int64)}
    for a in range(200, 1700):
        rows[(a, a % 7)] = np.array([(a * 31) % E], np.int64)
    keys = sorted(rows)
    ip = np.zeros(len(keys) + 1, np.int64)
    ip[1:] = np.cumsum([len(rows[k]) for k in keys])
    return dict(e1=np.array([k[0] for k in keys], np.int64), rel=np.array([k[1] for k in keys], np.int64), tail_indptr=ip,
                tail_idx=np.concatenate([rows[k] for k in keys]))


def _skewed_batch(md, kf, B, seed):
    """About half of the keys absent; the long rows first, last and adjacent; the 3,000-tail key five times; both ends of the key
    range; half of the targets drawn from their own rows."""
    E, R = int(md["num_ent"]), int(md["num_rel"])
    rng = np.random.default_rng(seed)
    a = rng.integers(200, 1700, B)
    e1, rel = a.copy(), a % 7
    absent = rng.random(B) < 0.5
    e1[absent], rel[absent] = rng.integers(5000, E - 1, int(absent.sum())), 3        # (no row of the index has e1 in [5000, E - 1))
    mid = B // 2
    for pos, key in ((0, LONG), (1, LONG2), (mid, LONG), (mid + 1, LONG), (mid + 2, LONG2), (mid + 3, LONG), (B - 2, LONG2), (B - 1, LONG),
                     (5, (0, 0)), (6, (E - 1, R - 1)), (7, (E - 1, 0)), (8, (0, R - 1))):
        e1[pos], rel[pos] = key
    assert int(((e1 == LONG[0]) & (rel == LONG[1])).sum()) == 5
    ip, ix = _np_filter(kf, md, e1, rel)
    e2 = rng.integers(0, E, B)
    own = np.flatnonzero((np.diff(ip) > 0) & (rng.random(B) < 0.5))
    e2[own] = ix[ip[own] + rng.integers(0, 1 << 30, own.size) % np.diff(ip)[own]]
    return e1, rel, e2


@pytest.fixture(scope="module")
def fb_x3(fb):
    md, p, kf = fb
    m = _model(md, p, score_mode="bf16x3").set_known_facts(**kf)
    yield m
    m.close()


@pytest.mark.parametrize("B", [1023, 1025, 2049])
def test_skewed_rows_x3(fb, fb_x3, B):
    md, _, kf = fb
    e1, rel, e2 = _skewed_batch(md, kf, B, seed=B)
    ip, _ = _answers_equal(fb_x3, kf, md, e1, rel, e2, "fb15k237 bf16x3 B=%d" % B)
    assert ip[-1] > 5 * 3000 and 0.3 < float((np.diff(ip) == 0).mean()) < 0.7


def test_skewed_rows_f32(fb):
    md, p, kf = fb
    m = _model(md, p, score_mode="f32").set_known_facts(**kf)
    e1, rel, e2 = _skewed_batch(md, kf, 1025, seed=1025)
    _answers_equal(m, kf, md, e1, rel, e2, "fb15k237 f32 B=1025")
    m.close()


# ---------------------------------------------------------------------------------------------------- 6. an entity shard
def test_sharded_handle_takes_the_whole_index(fb):
    md, p, kf = fb
    E = int(md["num_ent"])
    m = _model(md, p, score_mode="bf16x3", shard=(E // 2, E)).set_known_facts(**kf)
    e1, rel, e2 = _skewed_batch(md, kf, 1025, seed=6)
    _answers_equal(m, kf, md, e1, rel, e2, "fb15k237 shard [E/2, E)", rank=False)      # (ranking needs the whole table: coper_rank)
    m.close()


# ---------------------------------------------------------------------------------------------------- 7. a buffer one entry short
def test_cap_one_short_writes_nothing(fb, fb_x3):
    md, _, kf = fb
    m, lib = fb_x3, _lib.load()
    e1, rel, _ = _skewed_batch(md, kf, 1025, seed=7)
    want_ip, want_ix = _np_filter(kf, md, e1, rel)
    nnz = int(want_ip[-1])
    de1, drel = torch.as_tensor(e1).to(DEV), torch.as_tensor(rel).to(DEV)
    ip = torch.zeros(1026, dtype=torch.int64, device=DEV)
    ix = torch.full((nnz,), -7, dtype=torch.int64, device=DEV)
    got = C.c_int64(-1)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.coper_known_filter(m._h, ptr(de1), ptr(drel), 1025, ptr(ip), ptr(ix), nnz - 1, C.byref(got), m._stream())
    torch.cuda.synchronize()
    assert rc == EINVAL and got.value == nnz
    assert bool((ix == -7).all()), "entries were written although cap < nnz"
    assert lib.coper_known_filter(m._h, ptr(de1), ptr(drel), 1025, ptr(ip), ptr(ix), nnz, C.byref(got), m._stream()) == 0
    _same_csr((ip, ix), (want_ip, want_ix), "cap == nnz")


# ---------------------------------------------------------------------------------------------------- 4. - 5. lifetime, validation
def _small():
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=4099, num_rel=12)
    return md, cdata.synthetic_params(md, 11)


def _train_batch(md, B, L, seed):
    rng = np.random.default_rng(seed)
    E, R = md["num_ent"], md["num_rel"]
    labels = np.zeros((B, L), np.float32)
    labels[:, 0] = 1.0
    return dict(e1=rng.integers(0, E, B), rel=rng.integers(0, R, B), lookup_values=rng.integers(0, E, (B, L)).astype(np.int32), e2_multi=labels)


def test_index_lifetime():
    lib = _lib.load()
    md, p = _small()
    qa, qb = cdata.synthetic_queries(md, 600, seed=1), cdata.synthetic_queries(md, 600, seed=2, mean_filter=9.0)
    kfa, kfb = cdata.known_facts_from_queries(qa), cdata.known_facts_from_queries(qb)
    # queries of both sets: each index holds about half of the keys
    e1, rel, e2 = (np.concatenate([qa[k][:150], qb[k][:150]]) for k in ("e1", "rel", "e2"))
    m = _model(md, {k: torch.as_tensor(np.array(v, np.float32)) for k, v in p.items()}, score_mode="bf16x3")
    m.train_init(seed=5)
    # everything the sequence below does WITHOUT an index, once: workspaces and the training state have their sizes
    m.train_step(_train_batch(md, 48, 37, seed=100))
    ip, ix = _np_filter(kfb, md, e1, rel)
    m.predict_topk(e1, rel, 10, ip, ix)
    m.rank_pass(e1, rel, e2, ip, ix)
    torch.cuda.synchronize()
    before = lib.coper_live_device_bytes()
    m.set_known_facts(**kfa)
    assert lib.coper_live_device_bytes() > before
    ipa, _ = _answers_equal(m, kfa, md, e1, rel, e2, "index A")
    m.set_known_facts(**kfb)
    ipb, _ = _answers_equal(m, kfb, md, e1, rel, e2, "index B")
    assert not np.array_equal(ipa, ipb)
    # a training step and a prepare leave the index alone; the answers are those of the explicit-CSR calls after the same step
    m.train_step(_train_batch(md, 48, 37, seed=101))
    m.prepare()
    _answers_equal(m, kfb, md, e1, rel, e2, "index B after a training step")
    m.set_known_facts(None)
    with pytest.raises(_lib.CoperError) as ei:
        m.known_filter(e1, rel)
    assert ei.value.code == ESTATE
    with pytest.raises(_lib.CoperError) as ei:
        m.predict_topk_known(e1, rel, 10)
    assert ei.value.code == ESTATE
    torch.cuda.synchronize()
    assert lib.coper_live_device_bytes() == before
    m.close()


@pytest.mark.parametrize("what", ["swapped keys", "duplicated key", "tail == num_ent", "descending tails", "indptr[n_keys] != nnz",
                                  "e1 == num_ent", "e1 == -1", "rel == num_rel", "indptr[0] == 1", "indptr decreases once"])
def test_device_validation_keeps_the_index_in_force(what):
    md, p = _small()
    E, R = md["num_ent"], md["num_rel"]
    q = cdata.synthetic_queries(md, 400, seed=4)
    kf = cdata.known_facts_from_queries(q)
    m = _model(md, p, score_mode="bf16x3").set_known_facts(**kf)
    bad = {k: v.copy() for k, v in cdata.known_facts_from_queries(cdata.synthetic_queries(md, 400, seed=9, mean_filter=8.0)).items()}
    long_row = int(np.argmax(np.diff(bad["tail_indptr"])))
    assert np.diff(bad["tail_indptr"])[long_row] >= 3
    at = bad["tail_indptr"][long_row]
    if what == "swapped keys":
        for k in ("e1", "rel"):
            bad[k][[10, 11]] = bad[k][[11, 10]]
        frag = "not ascending"
    elif what == "duplicated key":
        bad["e1"][21], bad["rel"][21] = bad["e1"][20], bad["rel"][20]
        frag = "twice"
    elif what == "tail == num_ent":
        bad["tail_idx"][bad["tail_indptr"][long_row + 1] - 1] = E          # (the last of its row: the row stays ascending)
        frag = "tail is outside"
    elif what == "descending tails":
        bad["tail_idx"][[at, at + 1]] = bad["tail_idx"][[at + 1, at]]
        frag = "strictly ascending"
    elif what == "indptr[n_keys] != nnz":
        bad["tail_indptr"][-1] += 1
        frag = "tail_indptr[n_keys] != nnz"
    elif what == "e1 == num_ent":
        bad["e1"][-1] = E                                                   # (the last key: the keys before it stay ascending)
        frag = "an e1 is outside"
    elif what == "e1 == -1":
        bad["e1"][0] = -1
        frag = "an e1 is outside"
    elif what == "rel == num_rel":
        bad["rel"][30] = R
        frag = "a rel is outside"
    elif what == "indptr[0] == 1":
        assert bad["tail_indptr"][1] >= 1                                   # (no decrease comes with it)
        bad["tail_indptr"][0] = 1
        frag = "tail_indptr[0] != 0"
    else:
        # boundary k is raised to boundary k + 2: it stays inside [0, nnz], the last entry stays nnz, and the only decrease is
        # from k to k + 1 (every row of a synthetic index holds its target: no two boundaries are equal)
        ip, k = bad["tail_indptr"], long_row + 1
        assert 0 < k and k + 2 < len(ip) and np.all(np.diff(ip) > 0)
        ip[k] = ip[k + 2]
        assert int((np.diff(ip) < 0).sum()) == 1 and ip[0] == 0 and ip[-1] == len(bad["tail_idx"]) and 0 <= ip.min() and ip.max() == ip[-1]
        frag = "tail_indptr decreases"
    with pytest.raises(_lib.CoperError) as ei:
        m.set_known_facts(**bad)
    assert ei.value.code == EINVAL and frag in str(ei.value), str(ei.value)
    if what not in ("swapped keys", "duplicated key", "tail == num_ent", "descending tails", "indptr[n_keys] != nnz"):
        assert "(1 place)" in str(ei.value), str(ei.value)
    e1, rel, e2 = q["e1"][:130], q["rel"][:130], q["e2"][:130]
    _answers_equal(m, kf, md, e1, rel, e2, "after a refused index (%s)" % what)
    m.close()
