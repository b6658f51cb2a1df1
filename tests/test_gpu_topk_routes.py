"""The routes of the top-k threshold kernel (kernels_topk_bf16.hip: k_topk_threshold_emit) that only long block axes reach, on
tables small enough to test in seconds (32-wide embeddings): the coarse route and its overflow fall-back (16,384 blocks and
more), the general route behind them, and the <8,2> instantiation (4,096 blocks and more, one 32-query strip per CU).  Every case
compares ids and values with the masked row's top-k of the mode's own logits, bit for bit, and the counts with the k = 0 call."""
import numpy as np
import pytest
import torch

from coper_amd import data as cdata

pytestmark = pytest.mark.gpu

TK_COARSE_MIN_BLOCKS, TK_BIN, TK_CL = 16384, 64, 128      # (csrc/coper_internal.h, csrc/kernels_topk_bf16.hip)
E_LONG = 32 * TK_COARSE_MIN_BLOCKS + 97                   # a ragged last group of coarse keys; the padding of n_eblk only rounds up
assert -(-E_LONG // 32) >= TK_COARSE_MIN_BLOCKS
Q_LONG = 48                                               # three 16-query strips: <4,4>


def _md(num_ent):
    return cdata.model_descriptors("fb15k237_cpg", num_ent=num_ent, num_rel=12, ent_emb_size=32, emb_h=4, emb_w=8)


def _model(md, p, mode):
    from coper_amd.models import ConvE
    return ConvE(md, device="cuda:0", score_mode=mode).load_parameters(p).prepare()


@pytest.fixture(scope="module")
def long_table():
    md = _md(E_LONG)
    return md, cdata.synthetic_params(md, 21), cdata.synthetic_queries(md, Q_LONG, seed=22, mean_filter=6.0, max_filter=40)


def _csr(rows):
    rows = [np.unique(np.asarray(r, np.int64)) for r in rows]          # the CSR contract: rows sorted ascending
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows)


def _check(O, m, h, e2, indptr, idx, ks, logits=None, sample=None):
    """rank_counts(k) against topk_filtered of the rows `sample` (all) of the model's own logits, for every k of ks; counts
    against the k = 0 call for all queries.  The reference is taken once, at the largest k: a top-k is a prefix of it."""
    tgt = m.target_scores(h, e2)
    ng0, ne0 = m.rank_counts(h, tgt, e2, indptr, idx)
    sample = np.arange(len(e2)) if sample is None else sample
    if logits is None:
        logits = m.score_all(h[torch.as_tensor(sample, device=h.device)]).cpu().numpy()
    sip, six = _csr([idx[indptr[i]:indptr[i + 1]] for i in sample])
    ev, ei = O.topk_filtered(logits, e2[sample], sip, six, max(ks))
    for k in ks:
        ng, ne, tv, ti = m.rank_counts(h, tgt, e2, indptr, idx, k=k)
        assert np.array_equal(ti.cpu().numpy()[sample], ei[:, :k]) and np.array_equal(tv.cpu().numpy()[sample], ev[:, :k]), k
        assert np.array_equal(ng.cpu().numpy(), ng0.cpu().numpy()) and np.array_equal(ne.cpu().numpy(), ne0.cpu().numpy()), k


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_coarse_route(oracle_chain, long_table, mode, monkeypatch):
    """16,388 blocks, ordinary filters: every strip finishes on the coarse route (m = k + filter entries <= TK_CL list entries
    reach tau_c only when ties are heavy); the <4,4> instantiation."""
    monkeypatch.setenv("COPER_TOPK_EXPAND", "1")      # (64-entity maxima would halve the block axis)
    md, p, q = long_table
    m = _model(md, p, mode)
    _check(oracle_chain, m, m.encode(q["e1"], q["rel"]), q["e2"], q["filt_indptr"], q["filt_idx"], (1, 10, 128))
    m.close()


def test_coarse_overflow_falls_back_to_three_sweeps(oracle_chain, long_table, monkeypatch):
    """Three queries of the first strip know 300 of their row's best entities: m = 310 list entries reach tau_c, more than TK_CL,
    and the strip -- its short-filter queries too -- starts again on the three-sweep route.  The other strips stay coarse."""
    monkeypatch.setenv("COPER_TOPK_EXPAND", "1")
    md, p, q = long_table
    m = _model(md, p, "bf16x3")
    h = m.encode(q["e1"], q["rel"])
    logits = m.score_all(h).cpu().numpy()
    rows = [list(q["filt_idx"][q["filt_indptr"][i]:q["filt_indptr"][i + 1]]) for i in range(Q_LONG)]
    for i in (1, 5, 9):
        rows[i] += list(np.argsort(-logits[i])[:300])
    indptr, idx = _csr(rows)
    assert (np.diff(indptr)[[1, 5, 9]] > TK_CL).all() and np.diff(indptr)[[0, 2, 15]].max() < TK_BIN
    _check(oracle_chain, m, h, q["e2"], indptr, idx, (10,), logits=logits)
    m.close()


@pytest.mark.parametrize("n_tied", [3000, 6000])
def test_exact_ties_at_the_threshold_on_a_long_axis(oracle_chain, long_table, n_tied, monkeypatch):
    """n_tied consecutive entities with a zero row and one large common bias: their blocks' maxima tie exactly at the
    threshold, and the ties must resolve to the lowest ids.  3,000: 94 blocks, more than TK_BIN, ranked in the coarse route's
    list.  6,000: 188 blocks, more than TK_CL: the coarse list overflows, then the fast path's bin list: the general route."""
    monkeypatch.setenv("COPER_TOPK_EXPAND", "1")
    md, p, q = long_table
    assert TK_BIN < n_tied // 32 and (n_tied // 32 > TK_CL) == (n_tied == 6000)
    p = dict(p)
    ent, bias = np.array(p["ent_emb"], np.float32), np.array(p["pred_bias"], np.float32)
    ent[100000:100000 + n_tied] = 0.0
    bias[100000:100000 + n_tied] = 30.0
    p["ent_emb"], p["pred_bias"] = ent, bias
    m = _model(md, p, "bf16x3")
    _check(oracle_chain, m, m.encode(q["e1"], q["rel"]), q["e2"], q["filt_indptr"], q["filt_idx"], (10,))
    m.close()


def test_wide_strips_two_histogram_copies(oracle_chain, monkeypatch):
    """4,098 blocks and 8,192 queries (one 32-query strip per CU and more): the <8,2> instantiation.  64 sampled queries against
    the reference (a logit is a function of its query and entity alone), all queries' counts against the k = 0 call."""
    monkeypatch.setenv("COPER_TOPK_EXPAND", "1")
    md = _md(131072 + 33)
    Q = 8192
    p = cdata.synthetic_params(md, 23)
    q = cdata.synthetic_queries(md, Q, seed=24, mean_filter=6.0, max_filter=40)
    m = _model(md, p, "bf16x3")
    sample = np.sort(np.random.default_rng(25).choice(Q, 64, replace=False))
    _check(oracle_chain, m, m.encode(q["e1"], q["rel"]), q["e2"], q["filt_indptr"], q["filt_idx"], (10,), sample=sample)
    m.close()
