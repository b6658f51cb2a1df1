"""coper_encode_rank called the way a foreign host binds it (include/coper_hip.h): raw device pointers and sizes through
ctypes, no routing by coper_amd's Python.  Filters with thousands of known answers inside one block of 32 queries -- the
case round 2 routed away from this entry point in Python: the library now spreads what exceeds a
workgroup's own share of its block over the chip (k_filter_excess_bf16x3).  Ranks must equal the closed form of
metrics.py:40-57 on the rank-defining logits AND the two-call path (coper_encode + coper_rank), bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from tests.helpers import rank_defining_logits

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _encode_rank(m, e1, rel, e2, indptr, idx, want_equal):
    from coper_amd import _lib
    B = len(rel)
    d_e1, d_rel, d_e2 = _dev(e1, torch.int64), _dev(rel, torch.int64), _dev(e2, torch.int64)
    d_ip, d_ix = _dev(indptr, torch.int64), _dev(idx if len(idx) else np.zeros(1, np.int64), torch.int64)
    ranks = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
    ne = torch.full((B,), -7, dtype=torch.int32, device="cuda:0") if want_equal else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = m._lib.coper_encode_rank(m._h, _p(d_e1), _p(d_rel), None, _p(d_e2), _p(d_ip), _p(d_ix), int(indptr[-1]), B, None, _p(ranks),
                                  _p(ne), stream)
    _lib.check(m._h, rc)
    torch.cuda.synchronize()
    return ranks.cpu().numpy()


def _two_calls(m, e1, rel, e2, indptr, idx):
    from coper_amd import _lib
    B = len(rel)
    d_e1, d_rel, d_e2 = _dev(e1, torch.int64), _dev(rel, torch.int64), _dev(e2, torch.int64)
    d_ip, d_ix = _dev(indptr, torch.int64), _dev(idx if len(idx) else np.zeros(1, np.int64), torch.int64)
    h = torch.empty((B, m.ent_emb_size), dtype=torch.float32, device="cuda:0")
    ranks = torch.empty((B,), dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(m._h, m._lib.coper_encode(m._h, _p(d_e1), _p(d_rel), B, None, _p(h), stream))
    _lib.check(m._h, m._lib.coper_rank(m._h, _p(h), _p(d_e2), _p(d_ip), _p(d_ix), int(indptr[-1]), B, _p(ranks), None, stream))
    torch.cuda.synchronize()
    return ranks.cpu().numpy(), h


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, (np.concatenate(rows) if indptr[-1] else np.zeros(0, np.int64)).astype(np.int64)


HEAVY_CASES = {
    # name: (queries, [(query, known answers to add)], every query of these blocks gets `per_query` more)
    "one_row_of_5000":            (200, [(7, 5000)], None),
    "rows_across_a_block_edge":   (200, [(31, 3000), (32, 4000), (150, 2000)], None),
    "whole_block_of_medium_rows": (200, [], (1, 300)),          # block 1: 32 queries x 300 entries = 9,600, none long by itself
    "last_partial_block":         (77, [(70, 5000), (76, 2500)], None),
    "every_block_listed":         (130, [(b, 1500) for b in range(0, 130, 32)], None),
    "exactly_the_own_share":      (64, [], None),                # block 0 trimmed to 352 and block 1 to 353 entries below: only block 1 is listed
    "single_query":               (1, [(0, 4000)], None),
}


@pytest.mark.parametrize("workload", ["fb15k237_cpg", "synth10m_cpg"])     # 13 and 16 k-steps: both instantiations of the tail kernels
@pytest.mark.parametrize("case", sorted(HEAVY_CASES))
def test_encode_rank_with_heavy_filter_blocks_through_the_c_abi(oracle_chain, workload, case):
    from coper_amd.models import ConvE
    Q, adds, block_fill = HEAVY_CASES[case]
    md = cdata.model_descriptors(workload, num_ent=6000, num_rel=20)
    params = cdata.synthetic_params(md, 3)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(params).prepare()
    E = md["num_ent"]
    q = cdata.synthetic_queries(md, Q, seed=11)
    rng = np.random.default_rng(21)
    rows = [q["filt_idx"][q["filt_indptr"][i]:q["filt_indptr"][i + 1]] for i in range(Q)]
    for i, n in adds:
        rows[i] = np.unique(np.concatenate([rows[i], rng.choice(E, n, replace=False)]))
    if block_fill:
        blk, per = block_fill
        for i in range(32 * blk, min(Q, 32 * blk + 32)):
            rows[i] = np.unique(np.concatenate([rows[i], rng.choice(E, per, replace=False)]))
    if case == "exactly_the_own_share":
        for i in range(64):
            rows[i] = np.unique(rng.choice(E, 40, replace=False))[:11 + (i == 40)]
        assert sum(len(r) for r in rows[:32]) == 352 and sum(len(r) for r in rows[32:]) == 353
    # what the dense mask of metrics.py:40-46 tolerates: the target inside its own row, and repeated ids (sorted: adjacent)
    for i in range(0, Q if case != "exactly_the_own_share" else 0, 3):
        rows[i] = np.sort(np.concatenate([rows[i], [q["e2"][i]], rows[i][:5]]))
    indptr, idx = _csr(rows)

    two, h = _two_calls(m, q["e1"], q["rel"], q["e2"], indptr, idx)
    logits = rank_defining_logits(oracle_chain, m, h, params)
    keep = ~cdata.csr_to_dense_filter(indptr, idx, E).astype(bool)
    keep[np.arange(Q), q["e2"]] = False
    tgt = logits[np.arange(Q), q["e2"]]
    want = 1 + ((logits > tgt[:, None]) & keep).sum(axis=1)
    assert np.array_equal(two, want)
    for rep in range(3):      # the list of blocks empties itself: the second and third pass start clean
        assert np.array_equal(_encode_rank(m, q["e1"], q["rel"], q["e2"], indptr, idx, want_equal=False), want), rep
    assert np.array_equal(_encode_rank(m, q["e1"], q["rel"], q["e2"], indptr, idx, want_equal=True), want)
    # a light pass after heavy ones on the same handle (nothing may be left in the list)
    light = cdata.synthetic_queries(md, Q, seed=12)
    a = _encode_rank(m, light["e1"], light["rel"], light["e2"], light["filt_indptr"], light["filt_idx"], want_equal=False)
    b, _ = _two_calls(m, light["e1"], light["rel"], light["e2"], light["filt_indptr"], light["filt_idx"])
    assert np.array_equal(a, b)
    m.close()


def test_heavy_blocks_inside_a_captured_graph(oracle_chain):
    """The excess launch is part of the captured sequence (sized by the capacity the capture was given) and its list is
    emptied on the device: replays with heavy and light CSRs alternate correctly."""
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=6000, num_rel=20)
    params = cdata.synthetic_params(md, 3)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(params).prepare()
    B, E = 96, md["num_ent"]
    rng = np.random.default_rng(5)
    run = m.capture_rank_pass(B, 12000, want_equal=False)      # ranks only: the sequence with the fused tail kernel
    for rep in range(4):
        q = cdata.synthetic_queries(md, B, seed=30 + rep)
        rows = [q["filt_idx"][q["filt_indptr"][i]:q["filt_indptr"][i + 1]] for i in range(B)]
        if rep % 2 == 0:
            rows[40 + rep] = np.unique(np.concatenate([rows[40 + rep], rng.choice(E, 5000, replace=False)]))
        indptr, idx = _csr(rows)
        got = run(q["e1"], q["rel"], q["e2"], indptr, idx)[0].cpu().numpy()
        want, _ = _two_calls(m, q["e1"], q["rel"], q["e2"], indptr, idx)
        assert np.array_equal(got, want), rep
    m.close()


def test_widen_ids_from_device_and_pinned_host_memory():
    """coper_widen_ids: int32 -> int64 for every length and alignment, the source on the device or in pinned host memory."""
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("nations_cpg")
    m = ConvE(md, device="cuda:0").load_parameters(cdata.synthetic_params(md, 0)).prepare()
    rng = np.random.default_rng(0)
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 100003):
        a = rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32)
        want = a.astype(np.int64)
        dev = torch.as_tensor(a).to("cuda:0")
        assert np.array_equal(m.widen_ids(dev).cpu().numpy(), want)
        pin = torch.as_tensor(a).pin_memory()
        assert np.array_equal(m.widen_ids(pin).cpu().numpy(), want)
        if n > 8:      # unaligned views take the element loop
            assert np.array_equal(m.widen_ids(dev[1:]).cpu().numpy(), want[1:])
            out = torch.empty(n, dtype=torch.int64, device="cuda:0")
            m.widen_ids(pin[3:], out=out[3:])
            assert np.array_equal(out[3:].cpu().numpy(), want[3:])
    with pytest.raises(ValueError):
        m.widen_ids(torch.zeros(4, dtype=torch.int32))          # pageable host memory is not device-mapped
    # the way back (coper_copy_out_i32): device -> pinned host / device, every length
    for n in (1, 5, 1024, 100003):
        a = torch.as_tensor(rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32)).to("cuda:0")
        host = torch.zeros(n, dtype=torch.int32).pin_memory()
        m.copy_out(a, host)
        torch.cuda.synchronize()
        assert torch.equal(host, a.cpu())
        if n > 8:
            host.zero_()
            m.copy_out(a[1:], host[1:])
            torch.cuda.synchronize()
            assert torch.equal(host[1:], a[1:].cpu()) and host[0] == 0
    m.close()


def test_host_batches_are_staged_through_one_pinned_buffer():
    """rank_pass fed NumPy arrays (what ranking_and_hits hands it) stages them through ConvE.stage_batch -- one pinned int32
    buffer, one coper_widen_ids launch, two buffers alternating -- and gives the ranks of the same batch fed as device tensors;
    batches of changing sizes reuse and grow the buffers."""
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=20)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(cdata.synthetic_params(md, 1)).prepare()
    for rep, Q in enumerate((700, 5, 9000, 700, 1, 2048, 9000)):
        q = cdata.synthetic_queries(md, Q, seed=40 + rep)
        if rep == 1:      # a batch without any known answer
            q["filt_indptr"] = np.zeros(Q + 1, np.int64)
            q["filt_idx"] = np.zeros(0, np.int64)
        host, _ = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], want_equal=False)
        dq = {k: torch.as_tensor(v).to("cuda:0") for k, v in q.items()}
        dev, _ = m.rank_pass(dq["e1"], dq["rel"], dq["e2"], dq["filt_indptr"], dq["filt_idx"], filt_nnz=len(q["filt_idx"]), want_equal=False)
        assert torch.equal(host, dev), (rep, Q)
    assert m._stage["pin"][0] is not None and m._stage["pin"][1] is not None
    # ids that do not fit int32 take the ordinary route (and are rejected by the id check, not mangled)
    big = np.array([2 ** 33], np.int64)
    t = m.stage_batch(big, big)
    assert int(t[0][0]) == 2 ** 33
    m.close()


def test_list_route_of_ranking_and_hits_stages_the_filter_with_native_checks():
    """`ranking_and_hits` on a plain list of CSR batches (coper_amd/metrics.py; the reference's loop, metrics.py:38-60): targets and
    filter go through ConvE.stage_csr -- narrowing, range check and rows-ascending check in one native pass (coper_pack_ids_i32) --,
    ranks and audit come back through one launch (coper_post_ranks_audit), the metrics from coper_hits_means.  Same results as the
    dataset route; batches with an UNSORTED filter row or an id beyond int32 take the general route and give the same ranks / the
    same id report as before."""
    from coper_amd.models import ConvE
    from coper_amd.metrics import ranking_and_hits
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=20)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(cdata.synthetic_params(md, 1)).prepare()
    q = cdata.synthetic_queries(md, 3000, seed=77)
    ds = cdata.EvalDataset(q, 512, md["num_ent"])
    want = ranking_and_hits(m, None, ds, "dataset", return_ranks=True)
    # a set larger than one device pass: equal chunks staged once, their passes queued back to back (the second call has the next
    # chunk's sort by relation done inside the running chunk's encoder launch: coper_group_next)
    for rep in range(3):
        m.profile(True); m.profile_read("group")
        got = ranking_and_hits(m, None, ds, "chunks", max_chunk=1000, return_ranks=True)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and np.array_equal(got[3], want[3]), rep
        assert m.profile_read("group")[1] == (3 if rep == 0 else 1), rep          # three chunks of 1,000
        m.profile(False)
    batches = list(ds)
    calls = []
    orig = m.stage_csr
    m.stage_csr = lambda *a: (calls.append(orig(*a)), calls[-1])[1]
    got = ranking_and_hits(m, None, batches, "list", return_ranks=True)
    assert calls and calls[-1] is not None                                   # the native route served it
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and np.array_equal(got[3], want[3])
    got = ranking_and_hits(m, None, batches[:1], "one batch", return_ranks=True)
    assert np.array_equal(got[3], want[3][:512]) and calls[-1] is not None
    # a filter row out of order: the general route sorts it (same ranks: the mask is a set)
    rev = [dict(b) for b in batches]
    b0 = rev[2]
    ip = np.asarray(b0["filt_indptr"])
    r = int(np.argmax(np.diff(ip)))
    assert ip[r + 1] - ip[r] >= 2
    ix = np.array(b0["filt_idx"], np.int64)
    ix[ip[r]:ip[r + 1]] = ix[ip[r]:ip[r + 1]][::-1]
    b0["filt_idx"] = ix
    got = ranking_and_hits(m, None, rev, "unsorted", return_ranks=True)
    assert calls[-1] is None and np.array_equal(got[3], want[3])
    # no known answers at all
    empty = [dict(b, filt_indptr=np.zeros(len(b["e1"]) + 1, np.int64), filt_idx=np.zeros(0, np.int64)) for b in batches[:2]]
    got = ranking_and_hits(m, None, empty, "no filter", return_ranks=True)
    ref, _ = m.rank_pass(np.concatenate([b["e1"] for b in empty]), np.concatenate([b["rel"] for b in empty]),
                         np.concatenate([b["e2"] for b in empty]), np.zeros(1025, np.int64), np.zeros(0, np.int64), want_equal=False)
    assert calls[-1] is not None and np.array_equal(got[3], ref.cpu().numpy())
    m.close()


@pytest.mark.parametrize("k", [0, 1, 10])
def test_shard_record_pack_and_merge_match_the_tensor_formulation(k):
    """coper_pack_shard_record / coper_merge_shard_records (step 3 of the entity-sharded exchange) against the torch expressions
    they replace in coper_amd/sharding.py: the same int64 record (counts, score bits, ids, audit row) and, from records of three
    shards, the same ranks, tie counts and candidate lists."""
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=20)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3", band_audit_period=1).load_parameters(cdata.synthetic_params(md, 1)).prepare()
    q = cdata.synthetic_queries(md, 700, seed=5)
    m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], want_equal=False)     # (leaves a real audit behind)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    world, B = 3, 701
    recs, parts = [], []
    for w in range(world):
        ng = torch.randint(0, 2 ** 31 - 1, (B,), generator=g, device="cuda:0", dtype=torch.int64).to(torch.int32)
        ne = torch.randint(0, 50, (B,), generator=g, device="cuda:0", dtype=torch.int64).to(torch.int32)
        tv = torch.randn((B, k), generator=g, device="cuda:0") if k else None
        if k:
            tv[5, 0] = float("-inf"); tv[7, k - 1] = -0.0
        ti = torch.randint(-1, 10 ** 7, (B, k), generator=g, device="cuda:0", dtype=torch.int64) if k else None
        want = torch.zeros((B + 1, 1 + 2 * k), dtype=torch.int64, device="cuda:0")
        want[:B, 0] = (ng.to(torch.int64) << 32) | ne.to(torch.int64)
        if k:
            want[:B, 1:1 + k] = tv.contiguous().view(torch.int32).to(torch.int64)
            want[:B, 1 + k:] = ti
        if w == 0:
            ratio, pairs = m.band_audit(reset=False)
            assert pairs > 0
            want[B, 0] = (int(np.float32(ratio).view(np.uint32)) << 32) | (min(int(pairs), 0x7fffffff) & 0xffffffff)
        rec = m.pack_shard_record(ng, ne, tv, ti, reset_audit=True)
        assert torch.equal(rec, want), (w, k)
        if w == 0:
            assert m.band_audit(reset=False) == (0.0, 0)                 # read and reset on the device
        recs.append(rec); parts.append((ng, ne))
    allrec = torch.stack(recs)
    ranks, ne_tot, vals, ids = m.merge_shard_records(allrec, world, B, k)
    a = allrec[:, :B, :]
    assert torch.equal(ranks, (1 + (a[:, :, 0] >> 32).sum(dim=0)).to(torch.int32))
    assert torch.equal(ne_tot, (a[:, :, 0] & 0xFFFFFFFF).sum(dim=0).to(torch.int32))
    if k:
        wv = a[:, :, 1:1 + k].to(torch.int32).view(torch.float32).permute(1, 0, 2).reshape(B, -1)
        wi = a[:, :, 1 + k:].permute(1, 0, 2).reshape(B, -1)
        assert torch.equal(vals.view(torch.int32), wv.contiguous().view(torch.int32)) and torch.equal(ids, wi)
    else:
        assert vals is None and ids is None
    m.close()


def test_owned_rows_pack_and_unpack_match_the_tensor_formulation():
    """coper_pack_owned_rows / coper_unpack_rows (step 1 of the entity-sharded exchange) against the indexing expressions they
    replace in coper_amd/sharding.py, on a model that holds a SHARD of the table."""
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=20)
    p = cdata.synthetic_params(md, 1)
    lo, hi = 1000, 2200
    m = ConvE(md, device="cuda:0", score_mode="bf16x3", shard=(lo, hi)).load_parameters(p).prepare()
    rng = np.random.default_rng(2)
    d = md["ent_emb_size"]
    for n, cap in ((0, 0), (0, 5), (1, 1), (37, 37), (500, 777)):
        ids = rng.integers(lo, hi, n)
        loc = torch.as_tensor(ids - lo, dtype=torch.int64, device="cuda:0")
        buf = m.pack_owned_rows(loc, cap, 0.625, 1.5)
        rows, bias = m.owned_rows(ids)
        want = torch.zeros((cap + 1, d + 1), device="cuda:0")
        want[0, 0], want[0, 1] = 0.625, 1.5
        if n:
            want[1:1 + n, :d] = rows
            want[1:1 + n, d] = bias
        assert torch.equal(buf, want), (n, cap)
    world, cap, B = 3, 40, 129
    g = torch.Generator(device="cuda:0").manual_seed(0)
    out = torch.randn((world * (cap + 1), d + 1), generator=g, device="cuda:0")
    t1 = torch.randint(0, world * (cap + 1), (B,), generator=g, device="cuda:0")
    t2 = torch.randint(0, world * (cap + 1), (B,), generator=g, device="cuda:0")
    g1, g2, b2 = m.unpack_rows(out, t1, t2)
    w1, w2 = out.index_select(0, t1), out.index_select(0, t2)
    assert torch.equal(g1, w1[:, :d]) and torch.equal(g2, w2[:, :d]) and torch.equal(b2, w2[:, d])
    m.close()


def test_band_audit_and_table_exponent_through_the_c_abi():
    """coper_band_audit / coper_band_audit_post / coper_set_x3_ent_absmax as a foreign host binds them (include/coper_hip.h):
    every count launch audited (band_audit_period = 1), the ratio read with a synchronisation and posted to pinned memory
    without one; the ratio is relative to the band's allowance (a band ten times wider: a ratio ten times smaller); the
    setter's refusal at prepare."""
    from coper_amd import _lib
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=5000, num_rel=24)
    p = cdata.synthetic_params(md, 3)
    q = cdata.synthetic_queries(md, 1500, seed=9)

    def model(**kw):
        m = ConvE(md, device="cuda:0", score_mode="bf16x3", band_audit_period=1, **kw)
        return m.load_parameters(p).prepare()

    m = model()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ratio, pairs = ctypes.c_float(-1.0), ctypes.c_int64(-1)
    _lib.check(m._h, m._lib.coper_band_audit(m._h, 1, ctypes.byref(ratio), ctypes.byref(pairs), stream))      # reset
    r1 = _encode_rank(m, q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], False)
    pin = torch.zeros(2, dtype=torch.int32).pin_memory()
    _lib.check(m._h, m._lib.coper_band_audit_post(m._h, 0, ctypes.c_void_p(pin.data_ptr()), stream))          # no reset, no sync
    _lib.check(m._h, m._lib.coper_band_audit(m._h, 1, ctypes.byref(ratio), ctypes.byref(pairs), stream))      # synchronises
    assert pairs.value > 0 and 0.0 < ratio.value <= 0.5, (ratio.value, pairs.value)
    assert float(pin[:1].view(torch.float32)[0]) == ratio.value and int(pin[1]) == pairs.value
    _lib.check(m._h, m._lib.coper_band_audit(m._h, 0, ctypes.byref(ratio), ctypes.byref(pairs), stream))
    assert ratio.value == 0.0 and pairs.value == 0                                                          # the reset took
    # a band 10x wider than the library's: the same errors measured against ten times the allowance.  (Round 5: every query's own
    # target is audited as well -- it is always inside its band -- so the pair count no longer follows the band's width, and a
    # NARROWER band speaks up too: before, it held too few competitors to sample the error at all.)
    ratio1, pairs1 = float(pin[:1].view(torch.float32)[0]), int(pin[1])
    m2 = model(rank_band_kappa=1e-5)
    r2 = _encode_rank(m2, q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], False)
    ratio2, pairs2 = m2.band_audit()
    assert pairs2 >= pairs1 and 0.0 < ratio2 < ratio1 / 3, (ratio1, pairs1, ratio2, pairs2)
    assert np.array_equal(r1, r2)            # (either band leaves the close comparisons to the same fp32 chain)
    m4 = model(rank_band_kappa=1e-8)         # a hundred times too narrow: the audit reads far above what it read at 1e-6
    _encode_rank(m4, q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], False)
    ratio4, pairs4 = m4.band_audit()
    assert pairs4 >= 256 and ratio4 > 20 * ratio1, (ratio1, pairs1, ratio4, pairs4)
    m4.close()
    # the f32 mode has no band: zeros from the read, ESTATE from the post
    m3 = ConvE(md, device="cuda:0", score_mode="f32").load_parameters(p).prepare()
    _lib.check(m3._h, m3._lib.coper_band_audit(m3._h, 1, ctypes.byref(ratio), ctypes.byref(pairs), stream))
    assert ratio.value == 0.0 and pairs.value == 0
    assert m3._lib.coper_band_audit_post(m3._h, 0, ctypes.c_void_p(pin.data_ptr()), stream) == 5
    # table-wide maximum: accepted when it covers the rows, refused at prepare when it does not
    assert m._lib.coper_set_x3_ent_absmax(m._h, ctypes.c_float(100.0)) == 0
    _lib.check(m._h, m._lib.coper_prepare(m._h, stream))
    r3 = _encode_rank(m, q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], False)
    assert np.array_equal(r3, r1)            # another power of two on the planes, the same ranks
    assert m._lib.coper_set_x3_ent_absmax(m._h, ctypes.c_float(1e-6)) == 0
    assert m._lib.coper_prepare(m._h, stream) == 1 and b"x3_ent_absmax" in m._lib.coper_last_error(m._h)
    assert m._lib.coper_set_x3_ent_absmax(m._h, ctypes.c_float(-1.0)) == 1
    for x in (m, m2, m3):
        x.close()


@pytest.mark.parametrize("workload", ["fb15k237_cpg", "wn18rr_cpg"])      # the job rides in the fused encoder launch / runs as a launch of its own
def test_stage_ids_next_brings_the_next_batch_in_beside_the_encoder(workload):
    """coper_stage_ids_next: a pinned int32 batch registered before pass n is on the device, widened, after pass n -- and pass
    n's ranks do not change."""
    from coper_amd import _lib
    from coper_amd.models import ConvE
    md = cdata.model_descriptors(workload, num_ent=4000)
    p = cdata.synthetic_params(md, 5)
    Q = 5000 if workload == "fb15k237_cpg" else 600
    q = cdata.synthetic_queries(md, Q, seed=11)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(p).prepare()
    base = _encode_rank(m, q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], False)
    rng = np.random.default_rng(0)
    for n in (1, 7, 4096, 123457):
        src = torch.as_tensor(rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32)).pin_memory()
        dst = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
        assert m._lib.coper_stage_ids_next(m._h, ctypes.c_void_p(src.data_ptr()), n, _p(dst)) == 0
        assert np.array_equal(dst.cpu().numpy(), np.full(n, -1))          # nothing happens until the next encoder launch
        r = _encode_rank(m, q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], False)
        assert np.array_equal(r, base)
        assert np.array_equal(dst.cpu().numpy(), src.numpy().astype(np.int64))
        # the job ran once: another pass leaves a changed destination alone
        dst.fill_(-3)
        _encode_rank(m, q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], False)
        assert np.array_equal(dst.cpu().numpy(), np.full(n, -3))
    assert m._lib.coper_stage_ids_next(m._h, None, 5, None) == 1
    m.close()


@pytest.mark.parametrize("workload,Q", [("fb15k237_cpg", 6000), ("fb15k237_cpg", 700), ("fb15k237_plain", 3000), ("wn18rr_cpg", 900)])
def test_group_next_sorts_the_next_batch_beside_the_encoder(workload, Q):
    """coper_group_next: a stream of DIFFERENT batches, each staged (coper_stage_ids_next) and sorted by relation (coper_group_next)
    inside the previous pass's encoder launch, its ranks posted (coper_post_i32_next) in the next one's: every pass returns the ranks
    a plain pass returns, only the first pass groups itself, and whatever breaks the chain (another batch in between, a withdrawn
    registration, device-resident ids without a staging job, out-of-range ids) falls back or clamps exactly like the plain path."""
    from coper_amd.models import ConvE
    md = cdata.model_descriptors(workload, num_ent=4000)
    p = cdata.synthetic_params(md, 5)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(p).prepare()
    keys = ("e1", "rel", "e2", "filt_indptr", "filt_idx")
    qs = [cdata.synthetic_queries(md, Q, seed=40 + i) for i in range(5)]
    base = [_encode_rank(m, q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], False) for q in qs]
    pins, views = [], []
    width = max(sum(int(np.asarray(q[k]).size) for k in keys) for q in qs)
    stages = [torch.empty(width, dtype=torch.int64, device="cuda:0") for _ in range(2)]
    for q in qs:
        sizes = [int(np.asarray(q[k]).size) for k in keys]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        pin = torch.empty(int(offs[-1]), dtype=torch.int32).pin_memory()
        for k, o, n in zip(keys, offs, sizes):
            pin[o:o + n].copy_(torch.as_tensor(np.asarray(q[k]).astype(np.int32)))
        pins.append(pin)
        views.append([{k: st[o:o + n] for k, o, n in zip(keys, offs, sizes)} for st in stages])
    ranks = [torch.empty(Q, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    hosts = [torch.full((Q,), -1, dtype=torch.int32).pin_memory() for _ in qs]
    m.profile(True)
    m.profile_read("group")
    m.widen_ids(pins[0], out=stages[0][:pins[0].numel()])
    for i in range(len(qs)):
        c = i & 1
        if i + 1 < len(qs):
            m.stage_next(pins[i + 1], stages[1 - c][:pins[i + 1].numel()])
            m.group_next(views[i + 1][1 - c]["e1"], views[i + 1][1 - c]["rel"])
        v = views[i][c]
        r, _ = m.rank_pass(v["e1"], v["rel"], v["e2"], v["filt_indptr"], v["filt_idx"], want_equal=False, out=ranks[c])
        m.post_next(r, hosts[i])
    m.post_flush()
    torch.cuda.synchronize()
    for i in range(len(qs)):
        assert np.array_equal(hosts[i].numpy(), base[i]), i
    _, launches = m.profile_read("group")
    assert launches == 1, launches                       # only the first pass sorted its own batch
    # ids that are already on the device (no staging job): the role reads the int64 arrays
    v0, v1 = views[0][0], views[1][1]
    m.widen_ids(pins[0], out=stages[0][:pins[0].numel()]); m.widen_ids(pins[1], out=stages[1][:pins[1].numel()])
    m.group_next(v1["e1"], v1["rel"])
    r0, _ = m.rank_pass(v0["e1"], v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False)
    r1, _ = m.rank_pass(v1["e1"], v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False)
    assert np.array_equal(r0.cpu().numpy(), base[0]) and np.array_equal(r1.cpu().numpy(), base[1])
    assert m.profile_read("group")[1] == 1
    # a different batch in between drops the prepared grouping; a withdrawn registration prepares nothing
    m.group_next(v1["e1"], v1["rel"])
    r0, _ = m.rank_pass(v0["e1"], v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False)
    r0b, _ = m.rank_pass(v0["e1"], v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False)
    r1, _ = m.rank_pass(v1["e1"], v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False)
    assert np.array_equal(r0b.cpu().numpy(), base[0]) and np.array_equal(r1.cpu().numpy(), base[1])
    assert m.profile_read("group")[1] == 3
    m.group_next(v1["e1"], v1["rel"])
    assert m._lib.coper_group_next(m._h, None, None, 0, 0) == 0
    r0, _ = m.rank_pass(v0["e1"], v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False)
    r1, _ = m.rank_pass(v1["e1"], v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False)
    assert np.array_equal(r1.cpu().numpy(), base[1]) and m.profile_read("group")[1] == 2
    # out-of-range relation / entity ids: clamped and counted like the grouping kernels do (coper_check_ids)
    bad = {k: t.clone() for k, t in v1.items()}
    bad["rel"][3] = md["num_rel"] * 2 + 7 if "num_rel" in md else 10 ** 6
    bad["rel"][5] = -4
    ref, _ = m.rank_pass(bad["e1"], bad["rel"], bad["e2"], bad["filt_indptr"], bad["filt_idx"], want_equal=False)
    ref = ref.cpu().numpy()
    n_ref = m.check_ids() if hasattr(m, "check_ids") else None
    m.group_next(bad["e1"], bad["rel"])
    m.rank_pass(v0["e1"], v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False)
    got, _ = m.rank_pass(bad["e1"], bad["rel"], bad["e2"], bad["filt_indptr"], bad["filt_idx"], want_equal=False)
    assert np.array_equal(got.cpu().numpy(), ref)
    if n_ref is not None:
        assert m.check_ids() == n_ref
    assert m._lib.coper_group_next(m._h, None, None, 5, 0) == 1
    # a pass captured into a hipGraph neither carries a registration nor consumes a prepared grouping: the registration made before
    # the capture is dropped, replays and eager passes around them return the plain ranks
    if Q <= 3000:
        qd = {k: np.asarray(t.cpu()) for k, t in v1.items()}
        m.group_next(v1["e1"], v1["rel"])
        run = m.capture_rank_pass(Q, len(qd["filt_idx"]) + 8, want_equal=False)
        for _ in range(2):
            got = run(qd["e1"], qd["rel"], qd["e2"], qd["filt_indptr"], qd["filt_idx"])[0].cpu().numpy()
            assert np.array_equal(got, base[1])
        r1, _ = m.rank_pass(v1["e1"], v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False)
        assert np.array_equal(r1.cpu().numpy(), base[1])
        m.group_next(v1["e1"], v1["rel"])                      # prepared by an eager pass, then a replay in between, then the consumer
        m.rank_pass(v0["e1"], v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False)
        got = run(qd["e1"], qd["rel"], qd["e2"], qd["filt_indptr"], qd["filt_idx"])[0].cpu().numpy()
        r1, _ = m.rank_pass(v1["e1"], v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False)
        assert np.array_equal(got, base[1]) and np.array_equal(r1.cpu().numpy(), base[1])
    # a prepared grouping does not survive coper_prepare or a growing workspace (the second sets are sized by it): the consumer groups
    # itself, and the chain works again afterwards
    m.profile(True); m.profile_read("group")
    m.group_next(v1["e1"], v1["rel"])
    m.rank_pass(v0["e1"], v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False)
    m._prepared = False
    m.prepare()
    r1, _ = m.rank_pass(v1["e1"], v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False)
    assert np.array_equal(r1.cpu().numpy(), base[1]) and m.profile_read("group")[1] == 2
    m.group_next(v1["e1"], v1["rel"])
    m.rank_pass(v0["e1"], v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False)
    qbig = cdata.synthetic_queries(md, 2 * Q + 300, seed=91)
    rbig, _ = m.rank_pass(qbig["e1"], qbig["rel"], qbig["e2"], qbig["filt_indptr"], qbig["filt_idx"], want_equal=False)     # (the workspace grows)
    r1, _ = m.rank_pass(v1["e1"], v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False)
    assert np.array_equal(r1.cpu().numpy(), base[1])
    m.profile_read("group")
    m.group_next(v1["e1"], v1["rel"])
    r0, _ = m.rank_pass(v0["e1"], v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False)
    r1, _ = m.rank_pass(v1["e1"], v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False)
    assert np.array_equal(r0.cpu().numpy(), base[0]) and np.array_equal(r1.cpu().numpy(), base[1]) and m.profile_read("group")[1] == 1
    # the pass that follows hands its entity rows over itself (e1_rows: what the entity-sharded ranker's encoder gets)
    rows0, rows1 = m.gather_entities(v0["e1"]), m.gather_entities(v1["e1"])
    plain1, _ = m.rank_pass(None, v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False, e1_rows=rows1)
    assert np.array_equal(plain1.cpu().numpy(), base[1])
    m.profile_read("group")
    m.group_next(None, v1["rel"], e1_rows=True)
    m.rank_pass(None, v0["rel"], v0["e2"], v0["filt_indptr"], v0["filt_idx"], want_equal=False, e1_rows=rows0)
    got1, _ = m.rank_pass(None, v1["rel"], v1["e2"], v1["filt_indptr"], v1["filt_idx"], want_equal=False, e1_rows=rows1)
    assert np.array_equal(got1.cpu().numpy(), base[1]) and m.profile_read("group")[1] == 1
    m.close()


@pytest.mark.parametrize("Q", [6000, 700])      # the two-launch grouping (the job rides in its first launch) / the single-workgroup one (a launch of its own)
def test_post_i32_next_copies_the_last_ranks_beside_the_next_grouping(Q):
    """coper_post_i32_next: the ranks of pass n, registered after it was queued, reach pinned host memory during pass n + 1 -- not
    before -- and pass n + 1's own ranks are not disturbed; a withdrawn registration copies nothing."""
    from coper_amd import _lib
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=4000)
    p = cdata.synthetic_params(md, 5)
    qa, qb = cdata.synthetic_queries(md, Q, seed=31), cdata.synthetic_queries(md, Q, seed=32)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(p).prepare()
    ra = _encode_rank(m, qa["e1"], qa["rel"], qa["e2"], qa["filt_indptr"], qa["filt_idx"], False)
    rb = _encode_rank(m, qb["e1"], qb["rel"], qb["e2"], qb["filt_indptr"], qb["filt_idx"], False)
    assert not np.array_equal(ra, rb)
    ranks = torch.empty((Q,), dtype=torch.int32, device="cuda:0")
    host = torch.full((Q,), -5, dtype=torch.int32).pin_memory()
    r1, _ = m.rank_pass(qa["e1"], qa["rel"], qa["e2"], qa["filt_indptr"], qa["filt_idx"], want_equal=False, out=ranks)
    m.post_next(ranks, host)
    torch.cuda.synchronize()
    assert np.array_equal(host.numpy(), np.full(Q, -5))                 # nothing is queued by the registration
    keep = ranks.clone()
    r2, _ = m.rank_pass(qb["e1"], qb["rel"], qb["e2"], qb["filt_indptr"], qb["filt_idx"], want_equal=False, out=ranks)
    torch.cuda.synchronize()
    assert np.array_equal(host.numpy(), ra) and np.array_equal(keep.cpu().numpy(), ra)    # pass n's ranks, copied before pass n + 1 wrote its own
    assert np.array_equal(ranks.cpu().numpy(), rb)
    # the job ran once; a withdrawn registration copies nothing; post_flush copies at once
    host.fill_(-9)
    m.post_next(ranks, host)
    assert m._lib.coper_post_i32_next(m._h, None, 0, None) == 0
    m.rank_pass(qa["e1"], qa["rel"], qa["e2"], qa["filt_indptr"], qa["filt_idx"], want_equal=False)
    torch.cuda.synchronize()
    assert np.array_equal(host.numpy(), np.full(Q, -9))
    m.post_next(ranks, host)
    m.post_flush()
    torch.cuda.synchronize()
    assert np.array_equal(host.numpy(), ranks.cpu().numpy())
    assert m._lib.coper_post_i32_next(m._h, None, 5, None) == 1
    m.close()


def test_band_policy_widens_and_reranks_a_too_narrow_band():
    """coper_band_policy: the audit ACTS.  A band a thousand times too narrow (rank_band_kappa = 1e-9, every
    count launch audited) must still return the fp32 chain's ranks from `ranking_and_hits`: the first pass's audit reads far
    above 1, the policy widens kappa by the power of two that covers the error seen and the pass is ranked again.  All three
    routes of the drop-in ranker (dataset object, list of CSR batches, generator of the reference's dense-mask batches)."""
    import ctypes
    from coper_amd import _lib
    from coper_amd.metrics import ranking_and_hits
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=40)
    p = cdata.synthetic_params(md, 5)
    q = cdata.synthetic_queries(md, 2048, seed=7)
    m32 = ConvE(md, device="cuda:0", score_mode="f32").load_parameters(p).prepare()
    want = ranking_and_hits(m32, None, cdata.EvalDataset(q, 512, md["num_ent"]), "f32", return_ranks=True)[3]
    for route in ("dataset", "list", "dense_generator"):
        m = ConvE(md, device="cuda:0", score_mode="bf16x3", rank_band_kappa=1e-9, band_audit_period=1).load_parameters(p).prepare()
        ds = cdata.EvalDataset(q, 512, md["num_ent"], dense_mask=(route == "dense_generator"))
        ranking_and_hits.band_actions = 0
        if route == "dataset":
            src = ds
        elif route == "list":
            src = list(ds)
        else:
            src = ({k: v for k, v in b.items() if k not in ("filt_indptr", "filt_idx")} for b in ds)
        got = ranking_and_hits(m, None, src, route, return_ranks=True)[3]
        assert np.array_equal(got, want), route
        assert ranking_and_hits.band_actions >= 1, route          # the policy did act
        act, kappa = m.band_policy(0.0, 0)                         # (no pairs: keep; reports the kappa now in force)
        assert act == 0 and kappa >= 64e-9, (route, kappa)
        # a second evaluation starts from the widened band: no re-rank needed, same ranks
        ranking_and_hits.band_actions = 0
        src2 = ds if route != "list" else list(ds)
        got2 = ranking_and_hits(m, None, src2, route, return_ranks=True)[3]
        assert np.array_equal(got2, want) and ranking_and_hits.last_band_audit[0] < 1.0
        m.close()
    # the entity-sharded ranker applies the same policy on the audit words it exchanges with its records (one shard here: no
    # process group; the two-rank form runs in tests/test_gpu_multirank.py)
    from coper_amd.sharding import EntityShardedRanker
    m = ConvE(md, device="cuda:0", score_mode="bf16x3", rank_band_kappa=1e-9, band_audit_period=1).load_parameters(p).prepare()
    ranking_and_hits.band_actions = 0
    got = ranking_and_hits(m, None, cdata.EvalDataset(q, 512, md["num_ent"]), "sharded", ranker=EntityShardedRanker(m), return_ranks=True)[3]
    assert np.array_equal(got, want)
    assert m.band_policy(0.0, 0)[1] >= 64e-9                      # (the ranker widened the handle's band)
    m.close()
    # the C entry point as a foreign host binds it: thresholds and the multiplier's arithmetic
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(p).prepare()
    act, kap = ctypes.c_int32(), ctypes.c_float()
    for ratio, n, want_act, want_kappa in ((0.4, 100, 0, 1e-6), (0.7, 100, 1, 2e-6), (0.9, 0, 0, 2e-6), (3.0, 5, 2, 32e-6), (float("nan"), 5, 0, 32e-6)):
        _lib.check(m._h, m._lib.coper_band_policy(m._h, ratio, n, ctypes.byref(act), ctypes.byref(kap)))
        assert act.value == want_act and abs(kap.value / want_kappa - 1) < 1e-6, (ratio, act.value, kap.value)
    m.prepare()                                                    # the multiplier is a fact about the arithmetic: it survives
    _lib.check(m._h, m._lib.coper_band_policy(m._h, 0.0, 0, ctypes.byref(act), ctypes.byref(kap)))
    assert abs(kap.value / 32e-6 - 1) < 1e-6
    m32f = ConvE(md, device="cuda:0", score_mode="f32").load_parameters(p).prepare()
    _lib.check(m32f._h, m32f._lib.coper_band_policy(m32f._h, 5.0, 10, ctypes.byref(act), ctypes.byref(kap)))
    assert act.value == 0 and kap.value == 0.0                     # no band in the fp32-exact mode
    for x in (m, m32, m32f):
        x.close()


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_one_handle_per_role(mode):
    """coper_config.role (round 6): a COPER_ROLE_ENCODE handle and a COPER_ROLE_SCORE handle over the same parameter tensors give
    the bits of a handle that is both; each refuses the other role's entry points with COPER_ESTATE; each holds only its own
    derived buffers (coper_live_device_bytes)."""
    from coper_amd import _lib
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=6000, num_rel=60)
    p = {k: torch.as_tensor(v).to("cuda:0") for k, v in cdata.synthetic_params(md, 2).items()}
    q = cdata.synthetic_queries(md, 900, seed=3)
    lib = _lib.load()
    base = lib.coper_live_device_bytes()
    both = ConvE(md, device="cuda:0", score_mode=mode).load_parameters(p).prepare()
    n_both = lib.coper_live_device_bytes() - base
    enc = ConvE(md, device="cuda:0", score_mode=mode, role="encode").load_parameters(p).prepare()
    n_enc = lib.coper_live_device_bytes() - base - n_both
    sco = ConvE(md, device="cuda:0", score_mode=mode, role="score").load_parameters(p).prepare()
    n_sco = lib.coper_live_device_bytes() - base - n_both - n_enc
    assert 0 < n_enc < n_both and 0 < n_sco < n_both and n_enc + n_sco < 1.1 * n_both, (n_both, n_enc, n_sco)
    h0 = both.encode(q["e1"], q["rel"])
    h1 = enc.encode(q["e1"], q["rel"])
    assert torch.equal(h0, h1)
    r0, ne0 = both.rank(h0, q["e2"], q["filt_indptr"], q["filt_idx"])
    r1, ne1 = sco.rank(h1, q["e2"], q["filt_indptr"], q["filt_idx"])
    assert torch.equal(r0, r1) and torch.equal(ne0, ne1)
    assert torch.equal(both.score_all(h0[:64]), sco.score_all(h0[:64]))
    tgt = sco.target_scores(h0, q["e2"])
    a = both.rank_counts(h0, both.target_scores(h0, q["e2"]), q["e2"], q["filt_indptr"], q["filt_idx"], k=7)
    b = sco.rank_counts(h0, tgt, q["e2"], q["filt_indptr"], q["filt_idx"], k=7)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    rows = both.gather_entities(q["e1"])
    assert torch.equal(enc.gather_entities(q["e1"]), rows) and torch.equal(sco.gather_entities(q["e1"]), rows)
    assert torch.equal(enc.encode(None, torch.as_tensor(q["rel"]).to("cuda:0"), e1_rows=rows), h0)
    # step 1's pack on either handle (parameter tensors only); a row number outside the shard is a zero row, never a clamped entity
    loc = torch.as_tensor([5, md["num_ent"] + 3, 17, -2], dtype=torch.int64, device="cuda:0")
    buf = sco.pack_owned_rows(loc, 6, 1.5, 2.5)
    assert torch.equal(buf, enc.pack_owned_rows(loc, 6, 1.5, 2.5))
    assert buf[0, 0].item() == 1.5 and buf[0, 1].item() == 2.5
    assert torch.equal(buf[1, :-1], p["ent_emb"][5]) and torch.equal(buf[3, :-1], p["ent_emb"][17]) and buf[1, -1] == p["pred_bias"][5]
    assert not buf[2].any() and not buf[4].any() and not buf[5:].any()
    for bad in (lambda: enc.score_all(h0[:4]), lambda: enc.rank(h0, q["e2"], q["filt_indptr"], q["filt_idx"]),
                lambda: enc.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"]),
                lambda: sco.encode(q["e1"], q["rel"]), lambda: sco.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"]),
                lambda: sco.train_init()):
        with pytest.raises(_lib.CoperError) as e:
            bad()
        assert e.value.code == 5, e.value
    for m in (both, enc, sco):
        m.close()
    assert lib.coper_live_device_bytes() == base


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_refused_workspace_leaves_a_handle_that_regrows(mode):
    """A workspace the card cannot hold (coper_reserve of 2^40 queries: the query permutation alone is 4 TiB, refused by hipMalloc
    as an ordinary error before any kernel sees it) is COPER_ENOMEM; the handle holds no more device memory than before, and its
    next pass regrows the whole workspace and ranks as a fresh handle on the same parameters does, bit for bit."""
    from coper_amd import _lib
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=40)
    p = {k: torch.as_tensor(v).to("cuda:0") for k, v in cdata.synthetic_params(md, 4).items()}
    q = cdata.synthetic_queries(md, 700, seed=5)
    args = (q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
    lib = _lib.load()
    import gc
    gc.collect()
    base = lib.coper_live_device_bytes()
    m = ConvE(md, device="cuda:0", score_mode=mode).load_parameters(p).prepare()
    first, _ = m.rank_pass(*args, want_equal=False)          # (the workspace exists: every buffer the reserve regrows was there)
    torch.cuda.synchronize()
    held = lib.coper_live_device_bytes()
    with pytest.raises(_lib.CoperError) as e:
        m.reserve(1 << 40)
    assert e.value.code == 6, e.value
    assert lib.coper_live_device_bytes() <= held
    got, _ = m.rank_pass(*args, want_equal=False)
    fresh = ConvE(md, device="cuda:0", score_mode=mode).load_parameters(p).prepare()
    ref, _ = fresh.rank_pass(*args, want_equal=False)
    assert torch.equal(got, ref) and torch.equal(first, ref)
    for x in (m, fresh):
        x.close()
    assert lib.coper_live_device_bytes() == base


@pytest.mark.parametrize("workload,G", [("fb15k237_cpg", 3), ("synth10m_cpg", 8), ("wn18rr_cpg", 4)])
def test_generated_weights_of_the_held_relations_only(workload, G):
    """coper_config.rel_mod_* (round 6): an encoder handle that holds the generated dense weights of the relations r with
    r mod G == g only -- what rank g of an entity-sharded evaluation encodes -- gives the bits of a handle that holds them all,
    in 1 / G of the weight memory; a query of another relation is counted by coper_check_ids; what the option does not serve is
    refused by coper_prepare."""
    from coper_amd import _lib
    from coper_amd.models import ConvE
    md = cdata.model_descriptors(workload, num_ent=3000)
    if workload == "synth10m_cpg":
        md["num_rel"] = 203                                      # (not a multiple of G: the last slots of some ranks stay empty)
    p = {k: torch.as_tensor(v).to("cuda:0") for k, v in cdata.synthetic_params(md, 7).items()}
    q = cdata.synthetic_queries(md, 1500, seed=8)
    lib = _lib.load()
    import gc
    gc.collect()
    base = lib.coper_live_device_bytes()
    full = ConvE(md, device="cuda:0", score_mode="bf16x3", role="encode").load_parameters(p).prepare()
    n_full = lib.coper_live_device_bytes() - base
    h_full = full.encode(q["e1"], q["rel"])
    rows = full.gather_entities(q["e1"])
    for g in range(G):
        part = ConvE(md, device="cuda:0", score_mode="bf16x3", role="encode", rel_mod=(G, g)).load_parameters(p)
        before = lib.coper_live_device_bytes()
        part.prepare()
        n_part = lib.coper_live_device_bytes() - before
        assert n_part < n_full * (1.0 / G + 0.15), (g, n_part, n_full)
        mine = np.nonzero(q["rel"] % G == g)[0]
        sel = torch.as_tensor(mine).to("cuda:0")
        h = part.encode(q["e1"][mine], q["rel"][mine])
        assert torch.equal(h, h_full[sel]), g
        assert part.check_ids() == 0
        h2 = part.encode(None, torch.as_tensor(q["rel"][mine]).to("cuda:0"), e1_rows=rows[sel].contiguous())     # (what sharding.py's step 2 calls)
        assert torch.equal(h2, h_full[sel]), g
        if g == 0:
            other = np.nonzero(q["rel"] % G != g)[0][:37]
            part.encode(q["e1"][other], q["rel"][other])
            assert part.check_ids() == len(other)
        part.close()
    full.close()
    assert lib.coper_live_device_bytes() == base
    # refused: the fp32-exact mode, a static dense layer
    bad = ConvE(md, device="cuda:0", score_mode="f32", rel_mod=(G, 0)).load_parameters(p)
    with pytest.raises(_lib.CoperError) as e:
        bad.prepare()
    assert e.value.code == 7
    bad.close()
    mdp = cdata.model_descriptors("fb15k237_plain", num_ent=500)
    bad = ConvE(mdp, device="cuda:0", score_mode="bf16x3", rel_mod=(2, 1)).load_parameters(cdata.synthetic_params(mdp, 1))
    with pytest.raises(_lib.CoperError) as e:
        bad.prepare()
    assert e.value.code == 7
    bad.close()
    with pytest.raises(_lib.CoperError):
        ConvE(md, device="cuda:0", score_mode="bf16x3", rel_mod=(4, 4))
    assert lib.coper_live_device_bytes() == base
