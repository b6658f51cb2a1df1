"""The half tail of the x3 summation order (coper_amd/csrc/bf16x3_chain.h): at d = 193 .. 200 the 13th k-step holds at most 8 real
values, and every kernel of the mode sums its three products in two K = 16 accumulation steps instead of three -- one 16x16x32
instruction in the count kernel, two chained 32x32x16 everywhere else.  d = 201, 208 (a full tail) and 256 (no tail) keep the order
they had.  What must hold at every one of them:

  * ranks and tie counts are the fp32 chain's on the same h, exactly (the C restatement of the chain, tests/helpers.py);
  * the pair kernel's targets == the tile kernel's logits (score_all) == score_lookup, bit for bit;
  * the top-k values are the mode's own masked logits, bit for bit, with 32- and with 64-entity block maxima;
  * the mode's logits stay within the bound tests/test_gpu_scale.py applies, the band audit at or below 0.5.

Shape: |E| = 1,100 -- three rows of 512 entities for the count kernel, the last partial -- and 160 queries: two query tiles, the
second holding 32.  One 32-query block carries more than 352 known answers (the excess role of the band launch), and five queries
get planted competitors whose chain logit equals the target's, or sits one ulp above or below it: copies of the target's row that
differ in ONE element of the last k-step alone, so the comparison the band hands to the chain hangs on the packed step."""
import functools

import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from tests.test_gpu_scale import AUDIT_BAR, BIAS_WEIGHT, KAPPA, REL_ERR_BAR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E, Q = 1100, 160
HALF = (193, 200)                      # take the half tail
SAME = (201, 208, 256)                 # full tail, full tail, no tail: unchanged
GRID = {193: (193, 1), 200: (10, 20), 201: (3, 67), 208: (13, 16), 256: (16, 16)}
SIGMAS = (1.0, 1e-3)
PLANT_Q = (0, 5, 40, 129, 159)         # both query tiles, first and last query, one inside the heavy block
PLANT_IDS = (7, 600, 1030, 1060, 1097)  # first of three consecutive ids per planted query: all three rows of 512, the table's end
HEAVY = range(32, 64)                  # the 32-query block with more than 352 known answers
HEAVY_PER_QUERY = 12


def _md(d):
    if d == 200:
        return cdata.model_descriptors("fb15k237_cpg", num_ent=E, num_rel=12)
    emb_h, emb_w = GRID[d]
    md = dict(cdata._COMMON)
    f = 1 if emb_w < 3 else 3
    md.update(num_ent=E, num_rel=6, ent_emb_size=d, rel_emb_size=8, emb_h=emb_h, emb_w=emb_w, conv_filter_height=f, conv_filter_width=f,
              conv_num_channels=8, context_rel_conv=None, context_rel_out=[])
    return md


def _model(md, p, **kw):
    from coper_amd.models import ConvE
    return ConvE(md, device=DEV, score_mode="bf16x3", band_audit_period=1, **kw).load_parameters(p).prepare()


def _queries(d, seed):
    """e1 / rel / e2 and a CSR filter: a few known answers per query, HEAVY_PER_QUERY more in the heavy block; no planted id is an
    e1 (the encoder never reads a planted row), a target or a known answer, and no planted query's target is in a row but its own."""
    rng = np.random.default_rng(seed)
    md = _md(d)
    reserved = np.concatenate([np.arange(s, s + 3) for s in PLANT_IDS])
    free = np.setdiff1d(np.arange(E), reserved)
    e2 = rng.choice(free, Q, replace=False)
    rows = []
    for i in range(Q):
        n = int(rng.integers(0, 6)) + (HEAVY_PER_QUERY if i in HEAVY else 0)
        known = rng.choice(np.setdiff1d(free, e2[list(PLANT_Q)]), n, replace=False)
        rows.append(np.unique(np.concatenate([known, e2[i:i + 1]])))
    ip = np.zeros(Q + 1, np.int64)
    ip[1:] = np.cumsum([len(r) for r in rows])
    assert ip[64] - ip[32] > 352
    return dict(e1=rng.choice(free, Q).astype(np.int64), rel=rng.integers(0, int(md["num_rel"]), Q).astype(np.int64), e2=e2.astype(np.int64),
                filt_indptr=ip, filt_idx=np.concatenate(rows).astype(np.int64))


def _one_ulp_rows(O, ent, bias, hq, t_id):
    """Copies of row t_id with ONE element of the last k-step moved by whole ulps so that the chain logit against hq sits exactly
    one ulp above / below the row's own, or None where no such element exists (a target logit far smaller than the chain's running
    sum: the chain's results are then spaced wider than the target's ulp)."""
    d = ent.shape[1]
    k_lo = 16 * ((d - 1) // 16)                    # the last k-step of 16: the packed step of a half tail
    t = O.score_chain(hq, ent[t_id:t_id + 1], bias[t_id:t_id + 1])[0, 0]
    steps = np.arange(-16384, 16385)
    # the lightest product first (an ulp of a heavy one can step over an ulp of the logit)
    for kk in k_lo + np.argsort(np.abs(ent[t_id, k_lo:d].astype(np.float64) * hq[0, k_lo:d]), kind="stable"):
        cand = np.repeat(ent[t_id:t_id + 1], len(steps), axis=0)
        moved = cand[:, kk].view(np.int32) + steps.astype(np.int32)        # (ulps of a float: steps of its bit pattern)
        cand[:, kk] = moved.view(np.float32)
        lg = O.score_chain(hq, cand, np.full(len(steps), bias[t_id], np.float32))[0]
        up = np.flatnonzero(lg == np.nextafter(t, np.float32(np.inf)))
        dn = np.flatnonzero(lg == np.nextafter(t, np.float32(-np.inf)))
        if len(up) and len(dn):
            return cand[up[0]].copy(), cand[dn[0]].copy()
    return None


def _plant(O, ent, bias, h, q):
    """For every planted query: three copies of its target's row and bias -- the first left as it is (a tie), the others one ulp of
    the chain logit above and below.  Where the query's drawn target admits no such neighbours, the next entity that does becomes
    its target (e2 and the query's own filter row follow)."""
    reserved = set(int(c) + j for c in PLANT_IDS for j in range(3))
    ip, ix = q["filt_indptr"], q["filt_idx"]
    for qi, c0 in zip(PLANT_Q, PLANT_IDS):
        row = ix[ip[qi]:ip[qi + 1]]
        old = int(q["e2"][qi])
        for t_id in [old] + [e for e in range(E) if e not in reserved and e not in set(row.tolist())]:
            rows = _one_ulp_rows(O, ent, bias, h[qi:qi + 1], t_id)
            if rows is not None:
                break
        assert rows is not None, "no entity admits one-ulp neighbours for query %d" % qi
        row[row == old] = t_id
        row.sort()
        q["e2"][qi] = t_id
        ent[c0] = ent[t_id]
        ent[c0 + 1], ent[c0 + 2] = rows
        bias[c0:c0 + 3] = bias[t_id]


@functools.lru_cache(maxsize=None)
def _case(d, sigma):
    """Tables at scale sigma, h fed directly, the planted rows, and the chain's logits of all of it -- computed once per (d, sigma)."""
    from oracle import coper_oracle as O
    md = _md(d)
    rng = np.random.default_rng(1000 * d + int(round(-np.log10(sigma))))
    p = dict(cdata.synthetic_params(md, seed=d))
    ent = (rng.standard_normal((E, d)) * sigma).astype(np.float32)
    bias = (rng.standard_normal(E) * 0.1 * sigma).astype(np.float32)
    h = (rng.standard_normal((Q, d)) * sigma).astype(np.float32)
    q = _queries(d, seed=d)
    _plant(O, ent, bias, h, q)
    p["ent_emb"], p["pred_bias"] = ent, bias
    return md, p, h, q, O.score_chain(h, ent, bias)


def _closed_form(xl, q):
    mask = cdata.csr_to_dense_filter(q["filt_indptr"], q["filt_idx"], E).astype(bool)
    tgt = xl[np.arange(Q), q["e2"]]
    keep = ~mask
    keep[np.arange(Q), q["e2"]] = False
    return 1 + ((xl > tgt[:, None]) & keep).sum(axis=1), ((xl == tgt[:, None]) & keep).sum(axis=1), keep


def _check_logit_bound(logits, chain, h, p, what):
    hn = np.linalg.norm(h.astype(np.float64), axis=1)
    emax = float(np.linalg.norm(p["ent_emb"].astype(np.float64), axis=1).max())
    bmax = float(np.abs(p["pred_bias"]).max())
    allow = np.maximum(KAPPA * (hn * emax + BIAS_WEIGHT * bmax), 1e-300)
    rel = float((np.abs(logits.astype(np.float64) - chain.astype(np.float64)).max(axis=1) / allow).max())
    print("%s: max |s_x3 - s_chain| = %.3f of the band's allowance" % (what, rel))
    assert rel <= REL_ERR_BAR, (what, rel)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("d", HALF + SAME)
def test_every_logit_of_the_mode_agrees_and_ranks_are_the_chains(oracle_chain, d, sigma, monkeypatch):
    md, p, h_np, q, chain = _case(d, sigma)
    what = (d, sigma)
    want, want_eq, keep = _closed_form(chain, q)
    # the planted rows did what they were planted for: a tie, one above, nothing from the one below
    for qi, c0 in zip(PLANT_Q, PLANT_IDS):
        t = chain[qi, q["e2"][qi]]
        assert chain[qi, c0] == t and chain[qi, c0 + 1] == np.nextafter(t, np.float32(np.inf)) and chain[qi, c0 + 2] == np.nextafter(t, np.float32(-np.inf))
    assert (want_eq[list(PLANT_Q)] >= 1).all()
    outs = {}
    for xf in ("1", "2"):      # block maxima per 32 and per 64 entities (the count kernel's GM = 1 and 2; KS16 = 13 and 16 hold both)
        monkeypatch.setenv("COPER_TOPK_EXPAND", xf)
        m = _model(md, p, role="score")
        h = torch.as_tensor(h_np, device=DEV)
        logits = m.score_all(h).cpu().numpy()
        if xf == "1":
            _check_logit_bound(logits, chain, h_np, p, "d=%d sigma=%g" % what)
            # pair kernel == tile kernel == lookup, bit for bit
            tgt = m.target_scores(h, q["e2"])
            assert np.array_equal(tgt[0].cpu().numpy(), logits[np.arange(Q), q["e2"]]), what
            assert np.array_equal(tgt[1].cpu().numpy(), chain[np.arange(Q), q["e2"]]), what
            lookup = np.random.default_rng(d).integers(0, E, (Q, 9)).astype(np.int32)
            lookup[:, 0] = E - 1
            lookup[list(PLANT_Q), 1] = np.asarray(PLANT_IDS, np.int32) + 1
            got = m.score_lookup(h, lookup).cpu().numpy()
            assert np.array_equal(got, np.take_along_axis(logits, lookup.astype(np.int64), axis=1)), what
            # ranks and tie counts: the count kernel (GM = 0), the band walk, its audit
            m.band_audit()
            r, ne = m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
            ratio, n_pairs = m.band_audit()
            print("d=%d sigma=%g: band audit %.3f over %d pairs" % (d, sigma, ratio, n_pairs))
            assert np.array_equal(r.cpu().numpy(), want), what
            assert np.array_equal(ne.cpu().numpy(), want_eq), what
            assert n_pairs > 0 and ratio <= AUDIT_BAR, (what, ratio, n_pairs)
            r0, _ = m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"], want_equal=False)
            assert np.array_equal(r0.cpu().numpy(), want), what
        else:
            assert np.array_equal(logits, outs["logits"]), what
            tgt = m.target_scores(h, q["e2"])
        outs["logits"] = logits
        # top-k launches: values == the mode's own masked logits, counts == the ranks
        masked = np.where(keep | (np.arange(E)[None, :] == q["e2"][:, None]), logits, -np.inf)
        order_all = np.lexsort((np.broadcast_to(np.arange(E), masked.shape), -masked), axis=1)
        for k in (1, 10):
            out = m.rank_counts(h, tgt, q["e2"], q["filt_indptr"], q["filt_idx"], k=k)
            order = order_all[:, :k]
            want_val = np.take_along_axis(masked, order, axis=1)
            assert np.array_equal(out[2].cpu().numpy(), want_val), (what, xf, k)
            fin = np.isfinite(want_val)
            assert np.array_equal(out[3].cpu().numpy()[fin], order[fin]), (what, xf, k)
            assert np.array_equal(1 + out[0].cpu().numpy(), want), (what, xf, k)
            assert np.array_equal(out[1].cpu().numpy(), want_eq), (what, xf, k)
        m.close()


@pytest.mark.parametrize("sigma", SIGMAS)
def test_rank_pass_at_d200_with_a_heavy_block_and_planted_neighbours(oracle_chain, sigma):
    """The fused pass (encoder, tail kernel, count kernel, band + excess launch) at d = 200: h is the encoder's, the planted rows are
    built against it, and the heavy block's entries beyond the tail kernel's own share go through the excess role."""
    O = oracle_chain
    d = 200
    md = _md(d)
    rng = np.random.default_rng(77)
    p = dict(cdata.synthetic_params(md, seed=3))
    p["ent_emb"] = (rng.standard_normal((E, d)) * sigma).astype(np.float32)
    p["pred_bias"] = (rng.standard_normal(E) * 0.1 * sigma).astype(np.float32)
    q = _queries(d, seed=5)
    m0 = _model(md, p)
    h = m0.encode(q["e1"], q["rel"])
    m0.close()
    h_np = np.ascontiguousarray(h.cpu().numpy())
    _plant(O, p["ent_emb"], p["pred_bias"], h_np, q)
    chain = O.score_chain(h_np, p["ent_emb"], p["pred_bias"])
    want, want_eq, _ = _closed_form(chain, q)
    assert (want_eq[list(PLANT_Q)] >= 1).all()
    m = _model(md, p)
    m.band_audit()
    r, _, h2 = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], want_equal=False, want_h=True)
    assert torch.equal(h2, h)                       # (no e1 is a planted row: the encoder saw none of them)
    assert np.array_equal(r.cpu().numpy(), want), sigma
    ratio, n_pairs = m.band_audit()
    print("rank_pass d=200 sigma=%g: band audit %.3f over %d pairs" % (sigma, ratio, n_pairs))
    assert n_pairs > 0 and ratio <= AUDIT_BAR, (sigma, ratio, n_pairs)
    r1, ne1 = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
    assert np.array_equal(r1.cpu().numpy(), want) and np.array_equal(ne1.cpu().numpy(), want_eq), sigma
    r2, ne2 = m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    assert np.array_equal(r2.cpu().numpy(), want) and np.array_equal(ne2.cpu().numpy(), want_eq), sigma
    m.close()
