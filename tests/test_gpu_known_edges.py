"""The known-facts index where tests/test_gpu_known.py does not reach: past one chunk of the scan (4,096 lengths), past one sweep of
the build's grid (4,096 workgroups of 256), at the lane, wave and workgroup edges of the gather, the refusals and the empty rows
of the build, the workspaces between calls, and a capturing stream.

Everything is integer work: the expected CSR is `tests.helpers.known_filter_np` of the HOST index (itself checked against a
brute-force oracle in tests/test_known_oracle.py), the expected answers those of the explicit-CSR calls fed that CSR, and every
comparison is exact and names the first differing query.  The lookup kernels see only num_ent and num_rel, so the model is the
cheapest with the key space needed: the plain ConvE at num_ent = 4,099 (4,099 * 474 = 1,942,926 possible keys)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from coper_amd import _lib
from coper_amd import data as cdata
from tests.helpers import GEOMETRY_LENGTHS, empty_row_indexes, geometry_index, known_filter_np as _np_filter, known_index, known_probe_queries
from tests.test_gpu_known import DEV, EINVAL, _answers_equal, _model, _same, _same_csr

EUNSUPPORTED = 7
SCAN_CHUNK = 4096                 # k_known_scan: lengths per iteration of its one workgroup
SWEEP = 4096 * 256                # k_known_build: elements per sweep of its grid (at most 4,096 workgroups of 256 threads)


def _md():
    return cdata.model_descriptors("fb15k237_plain", num_ent=4099)


@pytest.fixture(scope="module")
def plain():
    """One handle for the tests that only replace the index; the tests of the state between calls make their own."""
    md = _md()
    m = _model(md, cdata.synthetic_params(md, 3), score_mode="bf16x3")
    yield md, m
    m.close()


# ---------------------------------------------------------------------------------------------------- 1. the scan's carry
@pytest.fixture(scope="module")
def carry_index():
    """3,000 rows of 0 .. 40 tails at EVEN keys: every odd key is absent."""
    md = _md()
    E, R = md["num_ent"], md["num_rel"]
    rng = np.random.default_rng(41)
    keys = 2 * np.sort(rng.choice(E * R // 2, 3000, replace=False))
    lens = rng.integers(0, 41, len(keys))
    assert lens.min() == 0 and lens.max() == 40
    return known_index({(int(k) // R, int(k) % R): np.sort(rng.choice(E, int(n), replace=False)) for k, n in zip(keys, lens)})


def _carry_batch(md, kf, B, seed):
    """B queries, a third of them absent (odd keys); the last one is the longest row, so that a last chunk of one entry has a sum."""
    E, R = md["num_ent"], md["num_rel"]
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(kf["e1"]), B)
    pick[-1] = int(np.argmax(np.diff(kf["tail_indptr"])))
    e1, rel = kf["e1"][pick].copy(), kf["rel"][pick].copy()
    absent = rng.random(B) < 1.0 / 3.0
    absent[-1] = False
    odd = 2 * rng.integers(0, E * R // 2, int(absent.sum())) + 1
    e1[absent], rel[absent] = odd // R, odd % R
    return e1, rel, absent


def _chunk_sums(ip):
    return np.add.reduceat(np.diff(ip), np.arange(0, len(ip) - 1, SCAN_CHUNK))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [4095, 4096, 4097, 8191, 8192, 8193, 12289, 20480])
def test_scan_carry(plain, carry_index, B):
    md, m = plain
    kf = carry_index
    m.set_known_facts(**kf)
    e1, rel, absent = _carry_batch(md, kf, B, seed=B)
    ip, ix = _np_filter(kf, md, e1, rel)
    # a dropped, reset or doubled carry changes indptr: every chunk has a sum of its own, none is 0
    sums = _chunk_sums(ip)
    assert len(sums) == (B + SCAN_CHUNK - 1) // SCAN_CHUNK and sums.min() > 0 and len(set(sums.tolist())) == len(sums), sums
    assert 0.28 < absent.mean() < 0.39 and np.all(np.diff(ip)[absent] == 0) and np.diff(ip).max() == 40
    _same_csr(m.known_filter(e1, rel), (ip, ix), "carry B=%d" % B)
    if B == 8193:
        rng = np.random.default_rng(B)
        e2 = rng.integers(0, md["num_ent"], B)
        own = np.flatnonzero((np.diff(ip) > 0) & (rng.random(B) < 0.5))
        e2[own] = ix[ip[own] + rng.integers(0, 1 << 30, own.size) % np.diff(ip)[own]]
        _answers_equal(m, kf, md, e1, rel, e2, "carry B=%d" % B)


@pytest.mark.gpu
def test_scan_carry_over_empty_chunks(plain, carry_index):
    """The carry has to survive chunks that add nothing, and a chunk of one entry has to receive it."""
    md, m = plain
    kf = carry_index
    m.set_known_facts(**kf)
    E, R = md["num_ent"], md["num_rel"]
    by_len = np.argsort(np.diff(kf["tail_indptr"]))
    long0, long1 = int(by_len[-1]), int(by_len[-2])
    n0, n1 = (int(np.diff(kf["tail_indptr"])[r]) for r in (long0, long1))
    assert n0 >= n1 >= 30

    def batch(B, present):
        odd = 2 * np.random.default_rng(B).integers(0, E * R // 2, B) + 1
        e1, rel = odd // R, odd % R
        for pos, row in present:
            e1[pos], rel[pos] = kf["e1"][row], kf["rel"][row]
        return e1, rel

    # only the first and the last of 12,289 queries are present: the chunks of the middle sum to 0
    e1, rel = batch(12289, [(0, long0), (12288, long1)])
    ip, ix = _np_filter(kf, md, e1, rel)
    assert _chunk_sums(ip).tolist() == [n0, 0, 0, n1] and ip[1] == n0 and ip[12288] == n0 and ip[12289] == n0 + n1
    _same_csr(m.known_filter(e1, rel), (ip, ix), "first and last of 12289")
    # the last full chunk is followed by ONE entry; the entries on both sides of each chunk edge are the only ones present
    e1, rel = batch(8193, [(4095, long0), (4096, long1), (8191, long1), (8192, long0)])
    ip, ix = _np_filter(kf, md, e1, rel)
    assert _chunk_sums(ip).tolist() == [n0, 2 * n1, n0] and ip[-1] == 2 * (n0 + n1)
    _same_csr(m.known_filter(e1, rel), (ip, ix), "chunk edges of 8193")
    # nothing present in the first two chunks, one entry in the third
    e1, rel = batch(8193, [(8192, long0)])
    ip, ix = _np_filter(kf, md, e1, rel)
    assert _chunk_sums(ip).tolist() == [0, 0, n0]
    _same_csr(m.known_filter(e1, rel), (ip, ix), "only the last of 8193")


# ---------------------------------------------------------------------------------------------------- 2. the gather's geometry
def _geometry_batches(names):
    """[(what, [row name, ...], check of the expected indptr)]: every batch is built by hand, the property it is built for is
    asserted on the NumPy side."""
    A, one = "absent", lambda i: ("one", i)
    ends = lambda ip: set(ip[1:].tolist())
    spaced = lambda n: [x for i in range(n) for x in (one(i), A)][:-1]
    return [
        ("row ends at 63, 64, 65", [63, 1, 1, 64, 2], lambda ip: {63, 64, 65} <= ends(ip)),
        ("row ends at 255, 256, 257", [255, 1, 1, 2, 1000], lambda ip: {255, 256, 257} <= ends(ip)),
        ("rows of 64 / 65 / 256 / 257 first", [64, 65, 127, 256, 257, 128, 129], lambda ip: {64, 129, 256, 512, 769} <= ends(ip)),
        ("a long row starts on lane 63", [63, 1000, 1], lambda ip: ip[1] % 64 == 63 and ip[2] - ip[1] == 1000),
        ("a long row ends on lane 0", [2] * 12 + [1, 1000, 1, 2], lambda ip: ip[13] == 25 and (ip[14] - 1) % 64 == 0 and (ip[14] - 1) % 256 == 0),
        ("a long row ends on lane 63, the next starts on lane 0", [2] * 12 + [1000, 1000], lambda ip: ip[12] == 24 and ip[13] % 64 == 0),
        ("64 one-entry owners, an absent query between every two", spaced(64), lambda ip: ip[-1] == 64 and len(ip) == 128),
        ("256 one-entry owners, an absent query between every two", spaced(256), lambda ip: ip[-1] == 256 and len(ip) == 512),
        ("300 one-entry owners, two absent queries after each", [x for i in range(300) for x in (one(i), A, "empty_mid")], lambda ip: ip[-1] == 300),
        ("total 1", [1], lambda ip: ip[-1] == 1),
        ("total 1 among empty queries", [A, "empty_first", 1, "empty_last", A], lambda ip: ip[-1] == 1),
        ("total 64, one row", [64], lambda ip: ip[-1] == 64),
        ("total 64, two rows", [A, 63, 1, A], lambda ip: ip[-1] == 64),
        ("total 256, one row", [256], lambda ip: ip[-1] == 256),
        ("total 256, three rows", [127, 128, A, 1], lambda ip: ip[-1] == 256),
        ("total 320", [64, 256], lambda ip: ip[-1] == 320),
        ("total 320, the other way round", [255, A, 65], lambda ip: ip[-1] == 320),
        ("70 empty queries lead, 300 trail", [A] * 35 + ["empty_first"] * 35 + [129, 2, 65] + ["empty_last", A] * 150,
         lambda ip: ip[70] == 0 and ip[73] == ip[-1] == 196),
        ("every length once", list(GEOMETRY_LENGTHS), lambda ip: ip[-1] == sum(GEOMETRY_LENGTHS)),
        ("every length once, descending", list(GEOMETRY_LENGTHS)[::-1], lambda ip: ip[-1] == sum(GEOMETRY_LENGTHS)),
    ]


@pytest.mark.gpu
def test_gather_geometry(plain):
    md, m = plain
    kf, names = geometry_index(md)
    m.set_known_facts(**kf)
    for what, rows, built_for in _geometry_batches(names):
        e1, rel = (np.array([names[r][c] for r in rows], np.int64) for c in (0, 1))
        ip, ix = _np_filter(kf, md, e1, rel)
        want_len = [r if isinstance(r, int) else 1 if isinstance(r, tuple) else 0 for r in rows]
        assert np.diff(ip).tolist() == want_len, what
        assert built_for(ip), "%s: the batch is not what it is built for: %s" % (what, ip[:20].tolist())
        _same_csr(m.known_filter(e1, rel), (ip, ix), what)
    # 20 seeded orders of one batch of about 200 queries over the same rows
    base = list(GEOMETRY_LENGTHS) * 3 + [("one", i) for i in range(100)] + ["absent"] * 40 + ["empty_first", "empty_mid", "empty_last"] * 8
    assert 190 <= len(base) <= 210
    for seed in range(20):
        rows = [base[i] for i in np.random.default_rng(seed).permutation(len(base))]
        e1, rel = (np.array([names[r][c] for r in rows], np.int64) for c in (0, 1))
        ip, ix = _np_filter(kf, md, e1, rel)
        assert ip[-1] == 3 * sum(GEOMETRY_LENGTHS) + 100
        _same_csr(m.known_filter(e1, rel), (ip, ix), "permutation %d" % seed)


# ---------------------------------------------------------------------------------------------------- 3. the build beyond one sweep
def _index_long_copy(md):
    """Index A: 400 rows of 3,000 tails -- 1.2 M tail entries, the copy loop of the build runs into its second sweep."""
    E, R = md["num_ent"], md["num_rel"]
    i = np.arange(400)
    tails = (np.arange(3000)[None, :] + (i * 7 % 1099)[:, None]).astype(np.int64)
    assert tails.max() < E
    return dict(e1=10 * i.astype(np.int64), rel=(i % R).astype(np.int64), tail_indptr=3000 * np.arange(401, dtype=np.int64), tail_idx=tails.ravel())


def _index_long_keys(md):
    """Index B: 1,150,000 rows of one tail -- the key loop of the build runs into its second sweep."""
    E, R = md["num_ent"], md["num_rel"]
    keys = np.sort(np.random.default_rng(43).choice(E * R, 1_150_000, replace=False)).astype(np.int64)
    return dict(e1=keys // R, rel=keys % R, tail_indptr=np.arange(len(keys) + 1, dtype=np.int64), tail_idx=(keys * 31) % E)


def _rows_around(kf, md, rows):
    """The keys of `rows` of the index and, between every two, the pair one key further (present or absent as it falls)."""
    E, R = md["num_ent"], md["num_rel"]
    key = (kf["e1"] * R + kf["rel"])[rows]
    both = np.stack([key, np.minimum(key + 1, E * R - 1)], axis=1).ravel()
    return both // R, both % R


def _refused(m, bad, frag):
    with pytest.raises(_lib.CoperError) as ei:
        m.set_known_facts(**bad)
    assert ei.value.code == EINVAL and frag in str(ei.value) and "(1 place)" in str(ei.value), str(ei.value)


def _sweep_queries(kf, md, element_row):
    """Queries from the first 100 keys, the last 100 keys and the rows on both sides of the row that holds element SWEEP."""
    n = len(kf["e1"])
    assert 3 <= element_row < n - 4
    return [("the first 100 keys", np.arange(100)), ("the last 100 keys", np.arange(n - 100, n)),
            ("rows on both sides of element 4096 * 256", np.arange(element_row - 3, element_row + 4))]


@pytest.mark.gpu
def test_build_long_copy_loop(plain):
    md, m = plain
    E = md["num_ent"]
    kf = _index_long_copy(md)
    nnz = len(kf["tail_idx"])
    assert nnz > SWEEP == 1048576 and len(kf["e1"]) + 1 < SWEEP          # (the sweeps beyond the first are those of the copy loop)
    element_row = int(np.searchsorted(kf["tail_indptr"], SWEEP, side="right") - 1)
    assert kf["tail_indptr"][element_row] <= SWEEP < kf["tail_indptr"][element_row + 1]
    assert m.set_known_facts(**kf) is m
    probes = [(what, _rows_around(kf, md, rows)) for what, rows in _sweep_queries(kf, md, element_row)]
    for what, (e1, rel) in probes:
        want = _np_filter(kf, md, e1, rel)
        assert want[0][-1] == 3000 * len(e1) // 2
        _same_csr(m.known_filter(e1, rel), want, "index A, " + what)
    # one violation each, beyond the first sweep
    bad = {k: v.copy() for k, v in kf.items()}
    at = int(kf["tail_indptr"][381]) - 1                                  # (the last of its row: the row stays ascending)
    assert at > SWEEP
    bad["tail_idx"][at] = E
    _refused(m, bad, "tail is outside")
    bad = {k: v.copy() for k, v in kf.items()}
    at = int(kf["tail_indptr"][390]) + 10
    assert at > SWEEP and at + 1 < kf["tail_indptr"][391]
    bad["tail_idx"][[at, at + 1]] = bad["tail_idx"][[at + 1, at]]
    _refused(m, bad, "strictly ascending")
    e1, rel = probes[2][1]
    _same_csr(m.known_filter(e1, rel), _np_filter(kf, md, e1, rel), "index A after two refusals")


@pytest.mark.gpu
def test_build_long_key_loop(plain):
    md, m = plain
    kf = _index_long_keys(md)
    n = len(kf["e1"])
    assert n > SWEEP == 1048576 and len(kf["tail_idx"]) == n
    assert m.set_known_facts(**kf) is m
    probes = [(what, _rows_around(kf, md, rows)) for what, rows in _sweep_queries(kf, md, SWEEP)]
    for what, (e1, rel) in probes:
        want = _np_filter(kf, md, e1, rel)
        assert len(e1) // 2 <= want[0][-1] < len(e1) and np.any(np.diff(want[0]) == 0)       # (the keys of the index, and absent ones)
        _same_csr(m.known_filter(e1, rel), want, "index B, " + what)
    bad = {k: v.copy() for k, v in kf.items()}
    at = 1_100_000
    assert at > SWEEP and at + 2 < n
    for k in ("e1", "rel"):
        bad[k][[at, at + 1]] = bad[k][[at + 1, at]]
    _refused(m, bad, "not ascending")
    e1, rel = probes[2][1]
    _same_csr(m.known_filter(e1, rel), _np_filter(kf, md, e1, rel), "index B after a refusal")


# ---------------------------------------------------------------------------------------------------- 4. empty rows
@pytest.mark.gpu
def test_empty_rows_are_accepted(plain):
    md, m = plain
    for name, kf in empty_row_indexes(md).items():
        assert m.set_known_facts(**kf) is m, name
        for seed in range(2):
            e1, rel = known_probe_queries(kf, md, seed)
            _same_csr(m.known_filter(e1, rel), _np_filter(kf, md, e1, rel), name)
    kf = geometry_index(md)[0]
    assert np.diff(kf["tail_indptr"])[[0, -1]].tolist() == [0, 0] and kf["e1"][-1] == md["num_ent"] - 1 and kf["rel"][-1] == md["num_rel"] - 1
    m.set_known_facts(**kf)
    e1, rel = known_probe_queries(kf, md, 0)
    _same_csr(m.known_filter(e1, rel), _np_filter(kf, md, e1, rel), "geometry index")


@pytest.mark.gpu
def test_descent_next_to_an_empty_row(plain):
    md, m = plain
    good = known_index({(1, 1): [5, 9], (1, 2): [], (1, 3): [3, 4]})
    m.set_known_facts(**good)
    e1, rel = known_probe_queries(good, md, 0)
    want = _np_filter(good, md, e1, rel)
    for what, rows in (("a descent inside the row that follows an empty row", {(1, 1): [5, 9], (1, 2): [], (1, 3): [7, 3]}),
                       ("a descent inside the row that follows two empty rows", {(1, 1): [5, 9], (1, 2): [], (1, 3): [], (1, 4): [2, 7, 3]}),
                       ("an equal adjacent pair inside a row", {(1, 1): [5, 9], (1, 2): [], (1, 3): [3, 3]}),
                       ("an equal pair at the end of the first row", {(1, 1): [5, 9, 9], (1, 2): [3, 4]})):
        bad = known_index(rows)
        with pytest.raises(_lib.CoperError) as ei:
            m.set_known_facts(**bad)
        assert ei.value.code == EINVAL and "strictly ascending" in str(ei.value) and "(1 place)" in str(ei.value), "%s: %s" % (what, ei.value)
        _same_csr(m.known_filter(e1, rel), want, "after " + what)


# ---------------------------------------------------------------------------------------------------- 5. the state between calls
@pytest.mark.gpu
def test_known_workspaces_between_calls(carry_index):
    lib = _lib.load()
    md = _md()
    E, R = md["num_ent"], md["num_rel"]
    m = _model(md, cdata.synthetic_params(md, 3), score_mode="bf16x3")
    big = carry_index
    rng = np.random.default_rng(51)
    # the small index: two keys of the big one with other tails, and one key the big one does not hold
    shared = [int(np.argmax(np.diff(big["tail_indptr"]))), 17]
    assert shared[0] != shared[1]
    small = known_index({(int(big["e1"][shared[0]]), int(big["rel"][shared[0]])): [1, 2, 3], (int(big["e1"][shared[1]]), int(big["rel"][shared[1]])): [],
                         (E - 1, R - 1): [0, 8, E - 1]})
    e1_big, rel_big, _ = _carry_batch(md, big, 5000, seed=5)
    absent = 2 * rng.integers(0, E * R // 2, 300) + 1                     # (odd keys: the big index holds none of them)
    b0 = (absent // R, absent % R, rng.integers(0, E, 300))
    b5000 = (e1_big, rel_big, rng.integers(0, E, 5000))
    b3 = (np.array([big["e1"][shared[0]], absent[0] // R, E - 1]), np.array([big["rel"][shared[0]], absent[0] % R, R - 1]), np.array([5, 6, 8]))
    pick = rng.integers(0, len(big["e1"]), 70)
    b70 = (np.concatenate([big["e1"][pick[:66]], big["e1"][shared], [E - 1, E - 1]]),
           np.concatenate([big["rel"][pick[:66]], big["rel"][shared], [R - 1, R - 2]]), rng.integers(0, E, 70))
    assert _np_filter(big, md, *b0[:2])[0][-1] == 0 and _np_filter(big, md, *b5000[:2])[0][-1] > 50000
    assert 40 <= _np_filter(big, md, *b3[:2])[0][-1] and _np_filter(small, md, *b3[:2])[0].tolist() == [0, 3, 3, 6]
    assert 6 <= _np_filter(small, md, *b70[:2])[0][-1] < _np_filter(big, md, *b70[:2])[0][-1]
    # everything the sequence does WITHOUT an index, once: the workspaces of the explicit-CSR calls have their sizes
    for kf, b in ((big, b0), (big, b5000), (big, b3), (small, b3), (small, b70)):
        ip, ix = _np_filter(kf, md, *b[:2])
        m.predict_topk(b[0], b[1], 10, ip, ix)
        m.rank_pass(b[0], b[1], b[2], ip, ix)
        m.rank_pass(b[0], b[1], b[2], ip, ix, want_equal=False)
    torch.cuda.synchronize()
    before = lib.coper_live_device_bytes()
    m.set_known_facts(**big)
    # 1. the first known call of the handle is a fused one that finds nothing
    ip, ix = _np_filter(big, md, *b0[:2])
    _same(m.predict_topk_known(b0[0], b0[1], 10), m.predict_topk(b0[0], b0[1], 10, ip, ix), "first call, total 0: predict_topk_known")
    _answers_equal(m, big, md, *b0, "total 0")
    # 2. - 3. a large batch, then a small one in the workspaces the large one left
    _answers_equal(m, big, md, *b5000, "5000 queries")
    _answers_equal(m, big, md, *b3, "3 queries after 5000")
    # 4. a much smaller index under the row numbers of the large one
    m.set_known_facts(**small)
    _answers_equal(m, small, md, *b3, "3 queries, small index")
    _answers_equal(m, small, md, *b70, "70 queries, small index")
    # 5. ranks only, then ranks and ties, of one batch
    ip, ix = _np_filter(small, md, *b70[:2])
    _same(m.rank_pass_known(*b70, want_equal=False), m.rank_pass(*b70, ip, ix, want_equal=False), "ranks only")
    _same(m.rank_pass_known(*b70, want_equal=True), m.rank_pass(*b70, ip, ix, want_equal=True), "ranks and ties after ranks only")
    m.set_known_facts(None)
    torch.cuda.synchronize()
    assert lib.coper_live_device_bytes() == before
    m.close()


# ---------------------------------------------------------------------------------------------------- 6. a capturing stream
def _hip_runtime():
    """The HIP runtime this process already runs on (torch and libcoper_hip.so share one), for the capture calls."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64.so" in os.path.basename(line.split()[-1])})
    assert paths, "no HIP runtime is loaded"
    hip = C.CDLL(paths[0])
    hip.hipStreamBeginCapture.argtypes, hip.hipStreamBeginCapture.restype = [C.c_void_p, C.c_int], C.c_int
    hip.hipStreamEndCapture.argtypes, hip.hipStreamEndCapture.restype = [C.c_void_p, C.POINTER(C.c_void_p)], C.c_int
    hip.hipGraphGetNodes.argtypes, hip.hipGraphGetNodes.restype = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)], C.c_int
    hip.hipGraphDestroy.argtypes, hip.hipGraphDestroy.restype = [C.c_void_p], C.c_int
    return hip


@pytest.mark.gpu
def test_known_calls_refuse_a_capturing_stream():
    lib = _lib.load()
    md = cdata.model_descriptors("nations_cpg")
    q0, q1 = cdata.synthetic_queries(md, 200, seed=2), cdata.synthetic_queries(md, 200, seed=3, mean_filter=6.0)
    kf0, kf1 = cdata.known_facts_from_queries(q0), cdata.known_facts_from_queries(q1)
    m = _model(md, cdata.synthetic_params(md, 3), score_mode="bf16x3").set_known_facts(**kf0)
    B, k = 64, 3
    e1, rel, e2 = (np.concatenate([q0[c][:32], q1[c][:32]]) for c in ("e1", "rel", "e2"))
    want0, want1 = _np_filter(kf0, md, e1, rel), _np_filter(kf1, md, e1, rel)
    assert want0[0][-1] > 0 and want1[0][-1] > 0 and not np.array_equal(want0[0], want1[0])
    cap = int(max(want0[0][-1], want1[0][-1]))
    dev = lambda a, dt=torch.int64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    de1, drel, de2 = dev(e1), dev(rel), dev(e2)
    d1 = {c: dev(v) for c, v in kf1.items()}
    ip = torch.full((B + 1,), -7, dtype=torch.int64, device=DEV)
    ix = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    tv = torch.full((B, k), -7.0, dtype=torch.float32, device=DEV)
    ti = torch.full((B, k), -7, dtype=torch.int64, device=DEV)
    ranks = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ne = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    nnz = C.c_int64(-1)
    # what the calls return outside a capture, and every workspace they need, before the capture
    _answers_equal(m, kf0, md, e1, rel, e2, "before the capture", k=k)
    side = torch.cuda.Stream(device=DEV)
    s = C.c_void_p(side.cuda_stream)
    calls = {
        "coper_set_known_facts": lambda: lib.coper_set_known_facts(m._h, ptr(d1["e1"]), ptr(d1["rel"]), ptr(d1["tail_indptr"]), ptr(d1["tail_idx"]),
                                                                   len(kf1["e1"]), len(kf1["tail_idx"]), s),
        "coper_known_filter": lambda: lib.coper_known_filter(m._h, ptr(de1), ptr(drel), B, ptr(ip), ptr(ix), cap, C.byref(nnz), s),
        "coper_predict_topk_known": lambda: lib.coper_predict_topk_known(m._h, ptr(de1), ptr(drel), None, B, k, ptr(tv), ptr(ti), s),
        "coper_encode_rank_known": lambda: lib.coper_encode_rank_known(m._h, ptr(de1), ptr(drel), None, ptr(de2), B, None, ptr(ranks), ptr(ne), s),
    }
    hip = _hip_runtime()
    torch.cuda.synchronize()
    live = lib.coper_live_device_bytes()
    assert hip.hipStreamBeginCapture(s, 0) == 0                           # hipStreamCaptureModeGlobal
    graph, n_nodes = C.c_void_p(), C.c_size_t(0)
    try:
        got = {name: (call(), (lib.coper_last_error(m._h) or b"").decode()) for name, call in calls.items()}
    finally:
        end = hip.hipStreamEndCapture(s, C.byref(graph))
    if graph.value:
        assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
        assert hip.hipGraphDestroy(graph) == 0
    torch.cuda.synchronize()
    assert end == 0, "the capture was invalidated: hipStreamEndCapture returned %d" % end
    for name, (rc, text) in got.items():
        assert rc == EUNSUPPORTED and name in text and "captured" in text, "%s returned %d: %s" % (name, rc, text)
    assert n_nodes.value == 0, "%d nodes were captured" % n_nodes.value
    assert lib.coper_live_device_bytes() == live
    for t in (ip, ix, ti, ranks, ne):
        assert bool((t == -7).all())
    assert bool((tv == -7.0).all())
    # the index in force is still the first, and the same calls on the same stream succeed now
    _same_csr(m.known_filter(e1, rel), want0, "after the capture")
    assert calls["coper_set_known_facts"]() == 0
    assert calls["coper_known_filter"]() == 0 and nnz.value == want1[0][-1]
    assert calls["coper_predict_topk_known"]() == 0
    assert calls["coper_encode_rank_known"]() == 0
    side.synchronize()
    _same_csr((ip, ix[:nnz.value]), want1, "coper_known_filter after the capture")
    _same((tv, ti), m.predict_topk(e1, rel, k, *want1), "coper_predict_topk_known after the capture")
    _same((ranks, ne), m.rank_pass(e1, rel, e2, *want1), "coper_encode_rank_known after the capture")
    m.close()
