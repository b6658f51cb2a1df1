"""The look-up role of the band launch past what tests/test_gpu_filter_bits.py reaches (kernels_score3_bf16.hip: band_lookup_body).

There Q <= 300: at most 19 ranges of 16 queries, one round of the scan for long ranges, long rows in the first two ranges only.
Here the role's own cut is under test: a wave owns TWO 16-query ranges, and a workgroup finds the long ranges of the launch in
batches of SCAN_BATCH ranges, its four waves taking the 64-range chunks of a batch in turn and exchanging what they found.  So: more
than 64 and more than 128 ranges (Q = 1,025, 1,040, 2,065), a partial last range, Q no multiple of 16 or 32, one range more than a
batch (Q = 16 SCAN_BATCH + 1), long rows in ranges 0, 63, 64, the last full and the partial last range, in the first and in the
second range of a wave, three long ranges side by side, an excess long enough to wrap round all waves of the role -- and no long
range at all, the benchmark's situation.  The reference of every case is the fp32-exact mode ranking the SAME h, bit for bit."""
import numpy as np
import pytest
import torch

from coper_amd import data as cdata

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = {198: (11, 18), 200: (10, 20), 208: (13, 16), 256: (16, 16)}   # d -> (emb_h, emb_w).  200: half tail of the x3 logit, 256: none;
#                                      208: a whole last k-step at 13 k-steps; 198: rows the tail kernel cannot load 16 bytes at a time
RANGE = 16                   # BL_QW: queries of one range
LOOKUP_OWN = 256             # BL_OWN: entries of a range its owner takes itself; the excess is dealt over all waves
SCAN_BATCH = 2048            # BL_SCAN_N: ranges a workgroup scans per batch (4 waves x 8 chunks of 64)
E_MAX = 1000


def _md(E, d, **kw):
    return cdata.model_descriptors("fb15k237_cpg", **dict(dict(num_ent=E, num_rel=14, ent_emb_size=d, emb_h=GRID[d][0], emb_w=GRID[d][1],
                                                               rel_emb_size=8), **kw))


def _model(md, p, mode="bf16x3", **kw):
    from coper_amd.models import ConvE
    return ConvE(md, device=DEV, score_mode=mode, **kw).load_parameters(p).prepare()


@pytest.fixture(scope="module")
def params_of():
    """d -> the parameters of the largest table (built once; the smaller table takes its first rows)."""
    cache = {}

    def get(d, E):
        if d not in cache:
            cache[d] = cdata.synthetic_params(_md(E_MAX, d), 5)
        return {k: (v[:E] if k in ("ent_emb", "pred_bias") else v) for k, v in cache[d].items()}

    yield get
    cache.clear()


@pytest.fixture(scope="module")
def handles_of(params_of):
    """(E, d, variant) -> (bf16x3 handle, f32 handle) on the same parameters, built once for the module."""
    cache = {}

    def get(E, d, twins=False):
        if (E, d, twins) not in cache:
            md = _md(E, d)
            p = dict(params_of(d, E))
            if twins:                      # odd rows repeat their even neighbours: the target's twin scores the target's logit exactly
                p["ent_emb"] = np.repeat(p["ent_emb"][0::2], 2, axis=0).copy()
                p["pred_bias"] = np.repeat(p["pred_bias"][0::2], 2).copy()
            cache[(E, d, twins)] = (md, _model(md, p), _model(md, p, "f32"))
        return cache[(E, d, twins)]

    yield get
    for _, m, m32 in cache.values():
        m.close(); m32.close()
    cache.clear()


def _csr(rows):
    ip = np.zeros(len(rows) + 1, np.int64)
    ip[1:] = np.cumsum([len(r) for r in rows])
    return ip, np.concatenate(rows).astype(np.int64)


def _ordinary(E, t, rng):
    return np.unique(np.concatenate([rng.integers(0, E, int(rng.integers(0, 12))), [t]])).astype(np.int64)


def _long(E, n, rng):
    """More than n entries, sorted, with adjacent duplicates (the recipe of test_gpu_filter_bits.py's kind 5)."""
    u = np.unique(rng.integers(0, E, 400))
    r = np.sort(np.repeat(u, -(-(n + 40) // len(u)))).astype(np.int64)
    assert len(r) > n
    return r


def _rows(E, e2, rng, long_ranges, all_entities_at):
    """Ordinary rows everywhere; in every range of `long_ranges` one or two rows of more than LOOKUP_OWN entries (at the first,
    a middle or the last query the range holds: the position moves with the range); the query `all_entities_at` lists every entity."""
    Q = len(e2)
    rows = [_ordinary(E, t, rng) for t in e2]
    lengths = (LOOKUP_OWN + 30, 700, 3000)              # one tile of excess, several, more tiles than the role has waves at Q ~ 1,000
    for i, r in enumerate(long_ranges):
        qa, qb = r * RANGE, min(r * RANGE + RANGE, Q)
        assert qa < Q, (r, Q)
        at = (qa, (qa + qb) // 2, qb - 1)[i % 3]
        rows[at] = _long(E, lengths[i % 3], rng)
        if i % 2 and qb - qa > 1:                        # two long rows in one range
            rows[qa if at != qa else qb - 1] = _long(E, LOOKUP_OWN + 1, rng)
    if all_entities_at is not None:
        rows[all_entities_at] = np.arange(E, dtype=np.int64)
    for r in long_ranges:
        assert sum(len(x) for x in rows[r * RANGE:r * RANGE + RANGE]) > LOOKUP_OWN
    return rows


def _check(m, m32, md, E, Q, long_ranges, all_entities_at, seed):
    q = cdata.synthetic_queries(md, Q, seed=seed)
    rows = _rows(E, q["e2"], np.random.default_rng(seed), long_ranges, all_entities_at)
    if not long_ranges and all_entities_at is None:      # no long range at all
        n = np.add.reduceat(np.array([len(r) for r in rows]), np.arange(0, Q, RANGE))
        assert n.max() <= LOOKUP_OWN
    ip, ix = _csr(rows)
    m.profile(True)
    m.profile_read("band_lookup"); m.profile_read("band_exact")
    r, none, h = m.rank_pass(q["e1"], q["rel"], q["e2"], ip, ix, want_equal=False, want_h=True)
    torch.cuda.synchronize()
    n_look, n_band = m.profile_read("band_lookup")[1], m.profile_read("band_exact")[1]
    m.profile(False)
    assert none is None and n_look == n_band == 1, (n_look, n_band)
    r = r.cpu().numpy()
    want = m32.rank(h, q["e2"], ip, ix)[0].cpu().numpy()
    assert np.array_equal(r, want), (E, Q, long_ranges, np.nonzero(r != want)[0][:8])
    if all_entities_at is not None:
        assert r[all_entities_at] == 1
    assert (r >= 1).all() and (r <= E).all()


def _layouts(Q):
    """(long ranges, the query that lists every entity) of one Q."""
    n_ranges = -(-Q // RANGE)
    last, last_full = n_ranges - 1, Q // RANGE - 1       # (the same range where Q is a multiple of 16)
    mid = n_ranges // 2
    return [
        (sorted({0, 63, 64, last_full, last}), 5 * RANGE + 3),       # a wave's first and second range, both sides of a 64-range chunk
        ([mid, mid + 1, mid + 2], Q - 1),                            # three long ranges side by side; every entity in the last query
        ([1, last], 0),                                              # odd ranges: the second range of a wave; every entity in query 0
        ([], None),                                                  # no long range: nothing for the scan to find
    ]


@pytest.mark.parametrize("Q", (1025, 1040, 2065))
@pytest.mark.parametrize("d", (200, 256))
@pytest.mark.parametrize("E", (257, 1000))
def test_long_rows_in_any_range_of_many(handles_of, E, d, Q):
    """Q = 1,025 (65 ranges, the last of one query), 1,040 (65 full ranges) and 2,065 (130 ranges, the last of one query), each with
    every layout of _layouts: ranks of an f32-mode handle on the same h, rank 1 where the row lists every entity, and the band launch
    carried the role."""
    md, m, m32 = handles_of(E, d)
    for i, (long_ranges, every) in enumerate(_layouts(Q)):
        _check(m, m32, md, E, Q, long_ranges, every, seed=10 * Q + i)


@pytest.mark.parametrize("case", ("both_batches", "side_by_side", "no_long_range"))
def test_one_range_more_than_a_scan_batch(handles_of, case):
    """Q = 16 SCAN_BATCH + 1: the scan takes a second batch for one range of one query.  Long rows in the last range of the first
    batch, in the lone range of the second, in ranges 0 and 63 / 64; three long ranges across the batches' border; then the same Q
    with no long range."""
    E, d, Q = 257, 200, RANGE * SCAN_BATCH + 1
    md, m, m32 = handles_of(E, d)
    if case == "both_batches":
        _check(m, m32, md, E, Q, [0, 63, 64, SCAN_BATCH - 1, SCAN_BATCH], 7 * RANGE + 1, seed=1)
    elif case == "side_by_side":
        _check(m, m32, md, E, Q, [SCAN_BATCH - 2, SCAN_BATCH - 1, SCAN_BATCH], Q - 1, seed=2)
    else:
        _check(m, m32, md, E, Q, [], None, seed=3)


# ---- the tail launch of these passes (kernels_tail_bf16.hip: k_finalize_targets_bf16x3): fragments, targets and bands


@pytest.mark.parametrize("Q", (1, 33, 129))
@pytest.mark.parametrize("d", sorted(GRID))
def test_tail_targets_near_the_top_and_inside_the_band(handles_of, d, Q):
    """One query, one block of 32 and one more, four blocks and one more (the grid is padded to 128 queries: blocks with no query at
    all), at 13 k-steps with a half last step (d = 200), a whole one (208) and rows read float by float (198), and at 16 (256).
    Targets among the top few logits of the f32 handle's row on a table whose odd rows repeat their even neighbours -- the twin is a
    known answer INSIDE the band -- as test_gpu_filter_bits.py plants them: a target, a band or a fragment off by one bit moves a
    rank.  Ranks of the f32 handle on the same h; the pass took the tail launch once and the look-up role."""
    E = 1000
    md, m, m32 = handles_of(E, d, twins=True)
    q = cdata.synthetic_queries(md, Q, seed=3 + Q)
    h0 = m.encode(q["e1"], q["rel"])
    top = torch.topk(m32.score_all(h0), 12, dim=1).indices.cpu().numpy()
    rng = np.random.default_rng(1000 * d + Q)
    e2 = top[np.arange(Q), rng.integers(0, 8, Q)]
    rows = []
    for i in range(Q):
        known = top[i, rng.random(12) < 0.4]
        rows.append(np.unique(np.concatenate([known, [e2[i], e2[i] ^ 1]])))       # the twin: inside the band
    ip, ix = _csr(rows)
    e2 = e2.astype(np.int64)
    m.profile(True)
    m.profile_read("tail"); m.profile_read("band_lookup")
    r, none, h = m.rank_pass(q["e1"], q["rel"], e2, ip, ix, want_equal=False, want_h=True)
    torch.cuda.synchronize()
    n_tail, n_look = m.profile_read("tail")[1], m.profile_read("band_lookup")[1]
    m.profile(False)
    assert none is None and n_tail == 1 and n_look == 1, (n_tail, n_look)
    want = m32.rank(h, e2, ip, ix)[0].cpu().numpy()
    r = r.cpu().numpy()
    assert np.array_equal(r, want), (d, Q, np.nonzero(r != want)[0][:8])
    # (the inputs are what they claim: the targets are near the top, and some known answers were above them)
    r0 = m32.rank(h, e2, np.zeros(Q + 1, np.int64), np.zeros(0, np.int64))[0].cpu().numpy()
    assert (r0 <= 12).all() and (r0 >= want).all()
    if Q >= 33:
        assert (r0 > want).sum() > Q // 4
