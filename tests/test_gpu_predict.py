"""coper_predict_topk on the GPU: the exact, filtered top-k of (e1, rel, ?) without a target.

The expected answer is never produced by the code under test: it is `score_all(h)` of a SECOND handle created with
score_mode="f32" on the same parameters (its logits are pinned bit-equal to the C chain and to the float64 oracle within 1e-3 by
tests/test_gpu_parity.py), masked with the CSR on the torch side and sorted by (-value, id) with a stable sort.  `h` is the tested
handle's own encode output, passed to both.  Every query of every case is compared: ids equal, values bit-equal, padding equal."""
import os

import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from coper_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AUDIT_BOUND = 0.5     # the bound the library's tests assert for the band audit (include/coper_hip.h: coper_band_audit)


def _model(md, p, **kw):
    from coper_amd.models import ConvE
    return ConvE(md, device=DEV, **kw).load_parameters(p).prepare()


def _expected(m32, h, ip, ix, k, chunk=4096):
    """Top-k of the f32 handle's masked rows, (value desc, id asc); (-inf, -1) padded.  ip / ix: host CSR or None (raw)."""
    lo, hi = m32.shard
    B = h.shape[0]
    vals, ids = [], []
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        lg = m32.score_all(h[b0:b1].contiguous())
        if ip is not None:
            cnt = np.diff(ip[b0:b1 + 1])
            rows = np.repeat(np.arange(b1 - b0), cnt)
            cols = np.asarray(ix[ip[b0]:ip[b1]], np.int64) - lo
            ok = (cols >= 0) & (cols < hi - lo)
            lg[torch.as_tensor(rows[ok], device=lg.device), torch.as_tensor(cols[ok], device=lg.device)] = float("-inf")
        sv, si = torch.sort(lg, dim=1, descending=True, stable=True)       # (stable over ascending ids: ties by id)
        kk = min(k, sv.shape[1])
        v = torch.full((b1 - b0, k), float("-inf"), device=lg.device)
        i = torch.full((b1 - b0, k), -1, dtype=torch.int64, device=lg.device)
        v[:, :kk] = sv[:, :kk]
        i[:, :kk] = si[:, :kk] + lo
        i[v == float("-inf")] = -1
        vals.append(v)
        ids.append(i)
    return torch.cat(vals), torch.cat(ids)


def _same(got, want, what):
    gv, gi = got
    wv, wi = want
    assert gv.dtype == torch.float32 and gi.dtype == torch.int64 and gv.shape == wv.shape and gi.shape == wi.shape, what
    bad = (gi != wi).any(dim=1) | (gv.view(torch.int32) != wv.view(torch.int32)).any(dim=1)
    n_bad = int(bad.sum())
    if n_bad:
        b = int(torch.nonzero(bad)[0])
        raise AssertionError("%s: %d of %d queries differ; first %d:\n got %s %s\nwant %s %s" % (
            what, n_bad, gi.shape[0], b, gi[b].tolist(), gv[b].tolist(), wi[b].tolist(), wv[b].tolist()))


def _check_all_forms(m, m32, q, ks, what, raw_too=True):
    """h form against the expectation, (e1, rel) form against the h form, raw and filtered, every k."""
    h = m.encode(q["e1"], q["rel"])
    ip, ix = q["filt_indptr"], q["filt_idx"]
    for k in ks:
        for filt in ((True, False) if raw_too else (True,)):
            a = (ip, ix) if filt else (None, None)
            got_h = m.predict_topk(None, None, k, a[0], a[1], h=h)
            _same(got_h, _expected(m32, h, a[0], a[1], k), "%s k=%d %s h-form" % (what, k, "filtered" if filt else "raw"))
            got_ids = m.predict_topk(q["e1"], q["rel"], k, a[0], a[1])
            _same(got_ids, got_h, "%s k=%d %s (e1, rel)-form against h-form" % (what, k, "filtered" if filt else "raw"))
    st = m.predict_stats()
    print("%s: %s" % (what, st))
    assert st["max_ratio"] <= AUDIT_BOUND, st
    return st


def _fwd_case(name):
    from oracle.gen_golden import FWD_CASES
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwd_%s.npz" % name))
    md = dict(cdata._COMMON)
    md.update(FWD_CASES[name][0])
    p = {k[6:]: g[k] for k in g.files if k.startswith("param:")}
    q = {k[2:]: g[k] for k in g.files if k.startswith("q:")}
    return md, p, q


# ---------------------------------------------------------------------------------------------------- 1. small fixtures
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("E", [14, 257, 4099])
def test_small_tables_every_k_raw_and_filtered_both_forms(E, mode):
    md = cdata.model_descriptors("nations_cpg") if E == 14 else cdata.model_descriptors("fb15k237_cpg", num_ent=E, num_rel=12)
    p = cdata.synthetic_params(md, 11)
    q = cdata.synthetic_queries(md, 300, seed=5)
    m, m32 = _model(md, p, score_mode=mode), _model(md, p, score_mode="f32")
    _check_all_forms(m, m32, q, (1, 3, 10, 128), "E=%d %s" % (E, mode))
    m.close()
    m32.close()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", ["plain", "cpg_fc", "cpg_fc_mlp", "cpg_conv_fc", "cpg_conv_only_concat", "lookup"])
def test_every_model_variant(name, mode):
    md, p, q = _fwd_case(name)
    m, m32 = _model(md, p, score_mode=mode), _model(md, p, score_mode="f32")
    _check_all_forms(m, m32, q, (1, 10), "%s %s" % (name, mode))
    m.close()
    m32.close()


# ---------------------------------------------------------------------------------------------------- 2. full size
@pytest.mark.parametrize("name,Q", [("fb15k237_cpg", 20480), ("wn18rr_cpg", 3072)])
def test_full_size_x3_exact_and_no_row_materialised(name, Q):
    lib = _lib.load()
    md = cdata.model_descriptors(name)
    p = cdata.synthetic_params(md, 0)
    q = cdata.synthetic_queries(md, Q, seed=1)
    m = _model(md, p, score_mode="bf16x3")
    h = m.encode(q["e1"], q["rel"])
    ip, ix = torch.as_tensor(q["filt_indptr"]).to(DEV), torch.as_tensor(q["filt_idx"]).to(DEV)
    torch.cuda.synchronize()
    before = lib.coper_live_device_bytes()
    got = m.predict_topk(None, None, 10, ip, ix, h=h)
    torch.cuda.synchronize()
    grew = lib.coper_live_device_bytes() - before
    st = m.predict_stats()
    print("%s Q=%d: ledger grew by %d bytes (row matrix: %d); %s" % (name, Q, grew, 4 * Q * md["num_ent"], st))
    assert grew < 4 * Q * md["num_ent"] // 4, (grew, 4 * Q * md["num_ent"])
    assert st["queries"] == Q and st["rescored"] >= 10 * (Q - st["unresolved"])
    assert st["max_ratio"] <= AUDIT_BOUND, st
    m32 = _model(md, p, score_mode="f32")        # (after the ledger was read: the counter is process-wide)
    _same(got, _expected(m32, h, q["filt_indptr"], q["filt_idx"], 10), "%s Q=%d" % (name, Q))
    m.close()
    m32.close()


# ---------------------------------------------------------------------------------------------------- 3. planted near-ties
def _plant(O, p, h0, ids_dup, ids_ulp):
    """Rows ids_dup = the same multiple of h0 (equal chain values: ties, decided by id); rows ids_ulp = that row with ONE coordinate
    moved by a few fp32 ulps so that its chain value is the neighbouring float.  Checked here on the CPU with the oracle's chain
    (float64 products: the margin of the planted rows over the rest)."""
    p = {k: np.array(v, copy=True) for k, v in p.items()}
    planted = np.concatenate([ids_dup, ids_ulp])
    rest = np.setdiff1d(np.arange(len(p["ent_emb"])), planted)
    rest_max = float((p["ent_emb"][rest].astype(np.float64) @ h0.astype(np.float64) + p["pred_bias"][rest]).max())
    hh = float(np.dot(h0.astype(np.float64), h0.astype(np.float64)))
    base = (h0 * np.float32((abs(rest_max) + 2.0) / hh)).astype(np.float32)
    chain = lambda rows: O.score_chain(np.ascontiguousarray(h0[None, :]), np.ascontiguousarray(rows), np.zeros(len(rows), np.float32))[0]
    v0 = chain(base[None, :])[0]
    assert v0 > rest_max + 1.0                          # the planted rows score highest
    up = np.nextafter(v0, np.float32(np.inf), dtype=np.float32)
    j = int(np.argmax(np.abs(h0 * base)))               # (base[j] h0[j] > 0: a larger |base[j]| is a larger product)
    row, steps = base.copy(), 0
    while chain(row[None, :])[0] == v0:
        steps += 1
        assert steps < 1 << 16
        row[j] = (base[j:j + 1].view(np.int32) + steps).view(np.float32)[0]
    assert chain(row[None, :])[0] == up, (chain(row[None, :])[0], v0, up)      # distinct by exactly one ulp of the logit
    p["ent_emb"][ids_dup] = base
    p["ent_emb"][ids_ulp] = row
    p["pred_bias"][planted] = 0.0
    assert (chain(p["ent_emb"][ids_dup]) == v0).all() and (chain(p["ent_emb"][ids_ulp]) == up).all()
    return p


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("n_dup", [40, 300])
def test_planted_near_ties_follow_the_chain(oracle_chain, mode, n_dup):
    O = oracle_chain
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=4099, num_rel=12)
    p = cdata.synthetic_params(md, 3)
    q = cdata.synthetic_queries(md, 96, seed=9)
    q["e1"][:48] = 7                      # a block of queries with one (e1, rel): one h, built to score the planted rows highest
    q["rel"][:48] = 2
    m = _model(md, p, score_mode=mode)
    h0 = m.encode(q["e1"][:1], q["rel"][:1]).cpu().numpy()[0]
    m.close()
    rng = np.random.default_rng(0)
    free = np.setdiff1d(np.arange(md["num_ent"]), np.unique(q["e1"]))      # (h depends on ent_emb[e1]: those rows stay)
    pick = rng.choice(free, n_dup + 40, replace=False)
    p2 = _plant(O, p, h0, np.sort(pick[:n_dup]), np.sort(pick[n_dup:]))
    m, m32 = _model(md, p2, score_mode=mode), _model(md, p2, score_mode="f32")
    h = m.encode(q["e1"], q["rel"])
    assert np.array_equal(h.cpu().numpy()[0], h0)
    m.predict_stats()
    for k in (1, 10, 39, 41, 60, 100, 128):           # the boundary inside the one-ulp group, at its end, inside the duplicates, beyond
        for a in ((q["filt_indptr"], q["filt_idx"]), (None, None)):
            _same(m.predict_topk(None, None, k, a[0], a[1], h=h), _expected(m32, h, a[0], a[1], k), "planted %s n_dup=%d k=%d" % (mode, n_dup, k))
    st = m.predict_stats()
    print("planted %s n_dup=%d: %s" % (mode, n_dup, st))
    if mode == "bf16x3":
        assert st["rescored"] > 0, st
        if n_dup == 300:
            assert st["unresolved"] >= 1, st
    m.close()
    m32.close()


# ---------------------------------------------------------------------------------------------------- 4. filter semantics
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_filter_semantics(mode):
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=700, num_rel=12)
    p = cdata.synthetic_params(md, 2)
    q = cdata.synthetic_queries(md, 64, seed=3)
    m, m32 = _model(md, p, score_mode=mode), _model(md, p, score_mode="f32")
    h = m.encode(q["e1"], q["rel"])
    B = len(q["e1"])
    raw_v, raw_i = m.predict_topk(None, None, 5, h=h)
    _same((raw_v, raw_i), _expected(m32, h, None, None, 5), "raw")
    # an empty CSR is the raw call
    _same(m.predict_topk(None, None, 5, np.zeros(B + 1, np.int64), np.zeros(0, np.int64), h=h), (raw_v, raw_i), "empty CSR")
    # the filter holds what would have been "the target" -- the best entity of every row -- and two more: none of them comes back
    top = raw_i.cpu().numpy()
    rows = [np.unique(np.concatenate([top[b, :1], top[b, 2:4]])) for b in range(B)]
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ix = np.concatenate(rows).astype(np.int64)
    fv, fi = m.predict_topk(None, None, 5, ip, ix, h=h)
    _same((fv, fi), _expected(m32, h, ip, ix, 5), "filtered")
    fi = fi.cpu().numpy()
    for b in range(B):
        assert not np.intersect1d(fi[b], rows[b]).size
        assert fi[b, 0] == top[b, 1]
    # a filter that leaves fewer than k entities: padded
    mdn = cdata.model_descriptors("nations_cpg")
    pn = cdata.synthetic_params(mdn, 1)
    qn = cdata.synthetic_queries(mdn, 40, seed=2)
    mn, mn32 = _model(mdn, pn, score_mode=mode), _model(mdn, pn, score_mode="f32")
    hn = mn.encode(qn["e1"], qn["rel"])
    ipn = (np.arange(41) * 9).astype(np.int64)
    ixn = np.concatenate([np.sort(np.random.default_rng(b).choice(14, 9, replace=False)) for b in range(40)]).astype(np.int64)
    gv, gi = mn.predict_topk(None, None, 10, ipn, ixn, h=hn)
    _same((gv, gi), _expected(mn32, hn, ipn, ixn, 10), "padded")
    assert (gi[:, 5:] == -1).all() and (gi[:, :5] >= 0).all() and torch.isinf(gv[:, 5:]).all()
    for x in (m, m32, mn, mn32):
        x.close()


# ---------------------------------------------------------------------------------------------------- 5. shards
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("world", [2, 4])
def test_shards_merge_to_the_unsharded_answer(world, mode):
    from coper_amd.sharding import merge_topk, shard_bounds
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=4099, num_rel=12)
    p = cdata.synthetic_params(md, 6)
    q = cdata.synthetic_queries(md, 200, seed=4)
    m, m32 = _model(md, p, score_mode=mode), _model(md, p, score_mode="f32")
    h = m.encode(q["e1"], q["rel"])
    for k in (3, 10):
        whole = m.predict_topk(None, None, k, q["filt_indptr"], q["filt_idx"], h=h)
        _same(whole, _expected(m32, h, q["filt_indptr"], q["filt_idx"], k), "unsharded k=%d" % k)
        vals, ids = [], []
        for g in range(world):
            ms = _model(md, p, score_mode=mode, shard=shard_bounds(md["num_ent"], world, g))
            v, i = ms.predict_topk(None, None, k, q["filt_indptr"], q["filt_idx"], h=h)
            lo, hi = ms.shard
            assert bool(((i == -1) | ((i >= lo) & (i < hi))).all())
            vals.append(v)
            ids.append(i)
            ms.close()
        _same(merge_topk(torch.cat(vals, dim=1), torch.cat(ids, dim=1), k), whole, "world %d k=%d" % (world, k))
    m.close()
    m32.close()


def test_entity_sharded_ranker_predicts_like_the_model():
    from coper_amd.sharding import EntityShardedRanker
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=40)
    p = cdata.synthetic_params(md, 4)
    q = cdata.synthetic_queries(md, 150, seed=8)
    m = _model(md, p, score_mode="bf16x3")
    er = EntityShardedRanker(m)
    want = m.predict_topk(q["e1"], q["rel"], 10, q["filt_indptr"], q["filt_idx"])
    _same(er.predict_topk(dict(e1=q["e1"], rel=q["rel"], filt_indptr=q["filt_indptr"], filt_idx=q["filt_idx"]), 10), want, "ranker filtered")
    _same(er.predict_topk(dict(e1=q["e1"], rel=q["rel"]), 10), m.predict_topk(q["e1"], q["rel"], 10), "ranker raw")
    m.close()


# ---------------------------------------------------------------------------------------------------- 6. factored handle
def test_factored_handle_on_its_own_h():
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3001, num_rel=30)
    p = cdata.synthetic_params(md, 5)
    q = cdata.synthetic_queries(md, 300, seed=6)
    m, m32 = _model(md, p, score_mode="bf16x3", dense="factored"), _model(md, p, score_mode="f32")
    _check_all_forms(m, m32, q, (10,), "factored")
    m.close()
    m32.close()


def test_fact_network_scorer_topk_is_the_top_of_forward(golden_dir):
    from coper_amd.fact_network import FactNetworkScorer
    g = np.load(os.path.join(golden_dir, "minerva_e2e.npz"))
    tag = "cpg"
    E, R, B, d1, d2, C, r_dim = (int(v) for v in g[tag + ":dims"])
    sd = {k.split(":sd:")[1]: torch.as_tensor(g[k]) for k in g.files if k.startswith(tag + ":sd:")}
    p32 = FactNetworkScorer(sd, torch.as_tensor(g[tag + ":ent"]), g[tag + ":rel"], d1, d2, cpg=True, device=DEV, score_mode="f32")
    for mode in ("f32", "bf16x3"):
        sc = FactNetworkScorer(sd, torch.as_tensor(g[tag + ":ent"]), g[tag + ":rel"], d1, d2, cpg=True, device=DEV, score_mode=mode)
        e1, r = (torch.as_tensor(g[tag + ":" + k].astype(np.int64)) for k in ("e1", "r"))
        val, idx = sc.predict_topk(e1, r, 5)
        assert tuple(val.shape) == (B, 5) and tuple(idx.shape) == (B, 5)
        # sigmoids of the exact top-5: the f32 handle's logits on this handle's h, sorted on the torch side
        h = sc.model.encode(e1.numpy(), r.numpy())
        wv, wi = _expected(p32.model, h, None, None, 5)
        assert torch.equal(idx, wi) and torch.equal(val, torch.sigmoid(wv))
        sc.close()
    p32.close()


# ---------------------------------------------------------------------------------------------------- 7. non-interference
def test_rank_passes_around_a_prediction_are_unchanged():
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3001, num_rel=30)
    p = cdata.synthetic_params(md, 7)
    q = cdata.synthetic_queries(md, 700, seed=12)
    q2 = cdata.synthetic_queries(md, 300, seed=13)

    def run(with_predict):
        m = _model(md, p, score_mode="bf16x3", band_audit_period=1)
        out = []
        if with_predict == "first":               # right after prepare(), nothing else run
            out.append(m.predict_topk(q2["e1"], q2["rel"], 10, q2["filt_indptr"], q2["filt_idx"]))
        r1, n1 = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
        a1 = m.band_audit(reset=False)
        if with_predict:
            out.append(m.predict_topk(q2["e1"], q2["rel"], 10, q2["filt_indptr"], q2["filt_idx"]))
        r2, n2 = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
        a2 = m.band_audit(reset=False)
        res = (r1.cpu().numpy(), n1.cpu().numpy(), a1, r2.cpu().numpy(), n2.cpu().numpy(), a2)
        m.close()
        return res, out

    base, _ = run(None)
    for mode in ("between", "first"):
        res, out = run(mode)
        for x, y in zip(res, base):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, mode
        for o in out[1:]:
            _same(o, out[0], "prediction repeated")
    m32, m = _model(md, p, score_mode="f32"), _model(md, p, score_mode="bf16x3")
    h = m.encode(q2["e1"], q2["rel"])
    _same(out[0], _expected(m32, h, q2["filt_indptr"], q2["filt_idx"], 10), "prediction right after prepare")
    m.close()
    m32.close()


def test_codes_on_a_prepared_handle():
    from coper_amd._lib import CoperError
    md = cdata.model_descriptors("nations_cpg")
    p = cdata.synthetic_params(md, 0)
    m = _model(md, p, score_mode="bf16x3")
    q = cdata.synthetic_queries(md, 8, seed=0)
    h = m.encode(q["e1"], q["rel"])
    with pytest.raises(CoperError) as e:
        m.predict_topk(None, None, 129, h=h)
    assert e.value.code == 7
    with pytest.raises(CoperError) as e:
        m.predict_topk(None, None, 0, h=h)
    assert e.value.code == 1
    v, i = m.predict_topk(None, None, 3, h=h[:0])
    assert v.shape == (0, 3) and i.shape == (0, 3)
    # out-of-range ids are clamped and counted like coper_encode's
    m.check_ids()
    bad_rel = q["rel"].copy()
    bad_rel[0] = md["num_rel"] + 5
    m.predict_topk(q["e1"], bad_rel, 3)
    assert m.check_ids() >= 1
    enc = _model(md, p, score_mode="bf16x3", role="encode")
    with pytest.raises(CoperError) as e:
        enc.predict_topk(q["e1"], q["rel"], 3)
    assert e.value.code == 7
    enc.close()
    m.close()


# ---------------------------------------------------------------------------------------------------- 9. the candidate pipeline's geometry
# d = 200 (13 k-steps: 32- and 64-entity block maxima are both instantiated), 5,000 entities, 300 queries: three query chunks of 128 (the
# last of 44) under COPER_TOPK_CHUNK_QUERIES=128.
def _chunk_table():
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=5000, num_rel=12)
    return md, cdata.synthetic_params(md, 11), cdata.synthetic_queries(md, 300, seed=5, mean_filter=6.0, max_filter=40)


def _predict_forms(m, q, h, k, filt):
    a = (q["filt_indptr"], q["filt_idx"]) if filt else (None, None)
    return m.predict_topk(None, None, k, a[0], a[1], h=h), m.predict_topk(q["e1"], q["rel"], k, a[0], a[1])


@pytest.fixture(scope="module")
def chunk_table():
    """The table, and per score mode the answers of a handle created with neither geometry variable set (one chunk, the default
    block-maximum granularity), computed once: [mode][k, filtered] -> (h form, (e1, rel) form)."""
    assert "COPER_TOPK_CHUNK_QUERIES" not in os.environ and "COPER_TOPK_EXPAND" not in os.environ
    md, p, q = _chunk_table()
    plain = {}
    for mode in ("f32", "bf16x3"):
        m = _model(md, p, score_mode=mode)
        h = m.encode(q["e1"], q["rel"])
        plain[mode] = {(k, filt): _predict_forms(m, q, h, k, filt) for k in (1, 10, 128) for filt in (True, False)}
        m.close()
    return md, p, q, plain


@pytest.mark.parametrize("mode,expand", [("bf16x3", "1"), ("bf16x3", "2"), ("f32", None)])
def test_several_query_chunks_and_both_block_maximum_granularities(chunk_table, mode, expand, monkeypatch):
    """The predictor's run of the candidate pipeline where the ranker's is tested (test_gpu_parity.py: test_pruned_topk_matches_masked_row_topk,
    test_topk_block_maxima_granularity): every answer equals the f32 handle's masked, sorted row, and is bit-equal to the answer of a
    handle of the same mode created with neither variable set (the variables are read per call and must not change under a handle
    that has made a top-k call, so that handle is another one)."""
    md, p, q, plain = chunk_table
    monkeypatch.setenv("COPER_TOPK_CHUNK_QUERIES", "128")
    if expand:
        monkeypatch.setenv("COPER_TOPK_EXPAND", expand)
    m, m32 = _model(md, p, score_mode=mode), _model(md, p, score_mode="f32")
    h = m.encode(q["e1"], q["rel"])
    for k in (1, 10, 128):
        for filt in (True, False):
            what = "%s expand=%s k=%d %s" % (mode, expand, k, "filtered" if filt else "raw")
            got_h, got_ids = _predict_forms(m, q, h, k, filt)
            _same(got_h, _expected(m32, h, q["filt_indptr"] if filt else None, q["filt_idx"] if filt else None, k), what + " h-form")
            _same(got_ids, got_h, what + " (e1, rel)-form against h-form")
            _same(got_h, plain[mode][k, filt][0], what + " h-form against the plain handle")
            _same(got_ids, plain[mode][k, filt][1], what + " (e1, rel)-form against the plain handle")
    st = m.predict_stats()
    print("%s expand=%s: %s" % (mode, expand, st))
    assert st["max_ratio"] <= AUDIT_BOUND, st
    m.close()
    m32.close()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_topk_workspaces_that_grow_between_calls_of_one_handle(mode):
    """rank_counts and predict_topk share the top-k workspaces of a handle: a sequence of calls in which they grow, are reused at a
    smaller size, and the first call is repeated, gives call by call the bits of the same call on a fresh handle."""
    md, p, q300 = _chunk_table()
    q40 = cdata.synthetic_queries(md, 40, seed=6, mean_filter=6.0, max_filter=40)
    q10 = cdata.synthetic_queries(md, 10, seed=7, mean_filter=6.0, max_filter=40)

    def counts(q, k):
        def run(m):
            h = m.encode(q["e1"], q["rel"])
            return m.rank_counts(h, m.target_scores(h, q["e2"]), q["e2"], q["filt_indptr"], q["filt_idx"], k=k)
        return run

    def predict(q, k):
        return lambda m: m.predict_topk(q["e1"], q["rel"], k, q["filt_indptr"], q["filt_idx"])

    steps = [("rank_counts k=4, 40 queries", counts(q40, 4)),
             ("predict_topk k=4, 40 queries: k + 4 blocks, the candidate group grows", predict(q40, 4)),
             ("rank_counts k=128, 300 queries: everything grows", counts(q300, 128)),
             ("predict_topk k=2, 10 queries: nothing grows", predict(q10, 2)),
             ("rank_counts k=4, 40 queries again", counts(q40, 4))]

    def bits(out):
        return [t.view(torch.int32).cpu() if t.dtype == torch.float32 else t.cpu() for t in out]

    m = _model(md, p, score_mode=mode)
    got = [bits(run(m)) for _, run in steps]
    m.close()
    for (what, run), g in zip(steps, got):
        fresh = _model(md, p, score_mode=mode)
        want = bits(run(fresh))
        fresh.close()
        assert len(g) == len(want) and all(torch.equal(a, b) for a, b in zip(g, want)), "%s %s: differs from a fresh handle" % (mode, what)
    assert all(torch.equal(a, b) for a, b in zip(got[4], got[0])), "%s: step 5 differs from step 1" % mode
