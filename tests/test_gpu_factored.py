"""MI355X: COPER_DENSE_FACTORED -- the generated dense layer at inference without the per-relation weight cache
(kernels_dense_factored_bf16.hip): h against the float64 oracle, ranks == the fp32 chain's on the handle's own h, batch invariance,
hostile inputs, inference after training steps, memory held, the drop-in surfaces, capture refused."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from tests.helpers import rank_defining_logits

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3      # the project's bars (tests/test_gpu_parity.py), not new numbers
H_TOL = 2e-4
EUNSUPPORTED = 7


def _model(md, params, dense="factored", **kw):
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0", score_mode="bf16x3", dense=dense, **kw)
    m.load_parameters(params)
    m.prepare()
    return m


def _fwd_case(golden_dir, name):
    from oracle.gen_golden import FWD_CASES
    g = np.load(os.path.join(golden_dir, "fwd_%s.npz" % name))
    md = dict(cdata._COMMON)
    md.update(FWD_CASES[name][0])
    p = {k[6:]: g[k] for k in g.files if k.startswith("param:")}
    q = {k[2:]: g[k] for k in g.files if k.startswith("q:")}
    return g, md, p, q


def _check_ranks_are_the_chains(O, m, h, p, q):
    """rank() == the reference ranker on the fp32 chain's logits of the handle's own h, ranks and tie counts, every query; and
    coper_encode_rank gives the same h and the same ranks."""
    chain = rank_defining_logits(O, m, h, p)
    ranks, ne = m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    ng_o, ne_o = O.rank_counts_c(chain, q["e2"], q["filt_indptr"], q["filt_idx"])
    assert np.array_equal(ranks.cpu().numpy(), 1 + ng_o) and np.array_equal(ne.cpu().numpy(), ne_o)
    r2, ne2, h2 = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], want_h=True)     # coper_encode_rank
    assert torch.equal(h2, h) and torch.equal(r2, ranks) and torch.equal(ne2, ne)
    return ranks.cpu().numpy()


@pytest.mark.parametrize("name", ["cpg_fc", "cpg_fc_mlp", "cpg_conv_fc"])
def test_golden_fixtures(golden_dir, oracle_chain, name):
    O = oracle_chain
    g, md, p, q = _fwd_case(golden_dir, name)
    m = _model(md, p)
    assert m.dense == "factored"
    h = m.encode(q["e1"], q["rel"])
    eh = np.abs(h.cpu().numpy() - g["f64:h"]).max()
    logits = m.score_all(h).cpu().numpy()
    el = np.abs(logits - g["f64:logits"]).max()
    print("%s factored: max |h - f64| = %.3e, max |logits - f64| = %.3e" % (name, eh, el))
    assert eh < H_TOL
    assert el < LOGIT_TOL
    _check_ranks_are_the_chains(O, m, h, p, q)
    m.close()


@pytest.mark.parametrize("name", ["plain", "lookup", "cpg_conv_only_concat"])
def test_static_and_looked_up_dense_layers_are_refused(golden_dir, name):
    from coper_amd import _lib
    from coper_amd.models import ConvE
    _, md, p, q = _fwd_case(golden_dir, name)
    with pytest.raises(_lib.CoperError) as ei:
        ConvE(md, device="cuda:0", score_mode="bf16x3", dense="factored")
    assert ei.value.code == EUNSUPPORTED and "COPER_DENSE_FACTORED" in str(ei.value)
    with pytest.raises(ValueError):
        ConvE(md, device="cuda:0", score_mode="bf16x3", dense="streamed")
    with pytest.raises(_lib.CoperError) as ei:     # the f32 mode of an otherwise fine configuration
        ConvE(_fwd_case(golden_dir, "cpg_fc")[1], device="cuda:0", score_mode="f32", dense="factored")
    assert ei.value.code == EUNSUPPORTED


def test_concat_rel_with_generated_dense_layer(oracle_chain):
    """No golden case has concat_rel with a generated dense layer: cpg_fc's descriptors plus concat_rel, synthetic parameters, against
    the float64 oracle.  A cached handle accepts the combination (checked here with the same bars), so the factored one serves it."""
    from oracle.gen_golden import FWD_CASES
    O = oracle_chain
    md = dict(cdata._COMMON)
    md.update(FWD_CASES["cpg_fc"][0])
    md.update(concat_rel=True)
    p = cdata.synthetic_params(md, seed=3)
    q = cdata.synthetic_queries(md, 48, seed=5, mean_filter=3.0, max_filter=16)
    st = O.forward(p, md, q["e1"], q["rel"], np.float64)
    lg64 = O.score_all(st["h"], p["ent_emb"].astype(np.float64), p["pred_bias"].astype(np.float64))
    for dense in ("cached", "factored"):
        m = _model(md, p, dense=dense)
        h = m.encode(q["e1"], q["rel"])
        eh = np.abs(h.cpu().numpy() - st["h"]).max()
        el = np.abs(m.score_all(h).cpu().numpy() - lg64).max()
        print("concat_rel %s: max |h - f64| = %.3e, max |logits - f64| = %.3e" % (dense, eh, el))
        assert eh < H_TOL and el < LOGIT_TOL
        _check_ranks_are_the_chains(O, m, h, p, q)
        m.close()


@pytest.mark.parametrize("name,Q", [("nations_cpg", 2000), ("fb15k237_cpg", 20480)])
def test_oracle_in_factored_form(oracle_chain, name, Q):
    """Full-size pass (Q queries in ONE rank_pass: several internal chunks at FB15k-237 shapes), every 97th query against the float64
    oracle in factored form.  Recorded, not gated: the share of sampled ranks equal to the float64 rank and max |h - h64|, for both
    dense modes."""
    O = oracle_chain
    md = cdata.model_descriptors(name)
    p = cdata.synthetic_params(md, 0)
    q = cdata.synthetic_queries(md, Q, seed=0)
    sub = np.arange(0, Q, 97)
    st = O.forward(p, md, q["e1"][sub], q["rel"][sub], np.float64, materialise=False)
    E64, b64 = p["ent_emb"].astype(np.float64), p["pred_bias"].astype(np.float64)
    lg64 = O.score_all(st["h"], E64, b64)
    for dense in ("factored", "cached"):
        m = _model(md, p, dense=dense)
        ranks, _, h = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], want_h=True)
        ranks = ranks.cpu().numpy()
        hs = h[torch.as_tensor(sub, device=h.device)].contiguous()
        eh = float(np.abs(hs.cpu().numpy() - st["h"]).max())
        logits = m.score_all(hs).cpu().numpy()
        err = float(np.abs(logits - lg64).max())
        n_same = 0
        if dense == "factored":
            assert eh < H_TOL, eh
            assert err < LOGIT_TOL, err
        for i, b in enumerate(sub):
            filt = q["filt_idx"][q["filt_indptr"][b]:q["filt_indptr"][b + 1]]
            t = lg64[i, q["e2"][b]]
            keep = np.ones(md["num_ent"], bool)
            keep[filt] = False
            keep[q["e2"][b]] = False
            others = lg64[i][keep]
            band = 2 * err + 1e-9
            lo_r, hi_r = 1 + int(np.sum(others > t + band)), 1 + int(np.sum(others > t - band))
            if dense == "factored":
                assert lo_r <= ranks[b] <= hi_r, (b, ranks[b], lo_r, hi_r)
            n_same += int(ranks[b] == 1 + int(np.sum(others > t)))
        print("%s %s: max |h - h64| = %.3e, max logit error %.3e, ranks equal to the float64 oracle's for %.4f of %d sampled queries"
              % (name, dense, eh, err, n_same / len(sub), len(sub)))
        if dense == "factored":      # the sampled ranks are the fp32 chain's on the handle's own h
            chain = O.score_chain(np.ascontiguousarray(hs.cpu().numpy()), p["ent_emb"], p["pred_bias"])
            ipl = q["filt_indptr"]
            sip = np.concatenate([[0], np.cumsum(ipl[sub + 1] - ipl[sub])])
            six = np.concatenate([q["filt_idx"][ipl[b]:ipl[b + 1]] for b in sub])
            ng_c, _ = O.rank_counts_c(chain, q["e2"][sub], sip, six)
            assert np.array_equal(ranks[sub], 1 + ng_c)
        m.close()


def test_batch_invariance(monkeypatch):
    """h[b] is a pure function of (e1[b], rel[b]): one batch, reversed, batches of 1 / 17 / 128, and two offsets inside a 9,000-query
    batch that crosses a chunk boundary -- the same bits."""
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000)
    p = cdata.synthetic_params(md, 1)
    m = _model(md, p)
    q = cdata.synthetic_queries(md, 300, seed=2)
    e1, rel = torch.as_tensor(q["e1"]), torch.as_tensor(q["rel"])
    h = m.encode(e1, rel).clone()
    assert torch.isfinite(h).all() and float(h.abs().max()) > 0
    assert torch.equal(m.encode(e1.flip(0), rel.flip(0)).flip(0), h)
    for bs in (1, 17, 128):
        n = 300 if bs > 1 else 40
        parts = [m.encode(e1[s:s + bs], rel[s:s + bs]).clone() for s in range(0, n, bs)]
        assert torch.equal(torch.cat(parts), h[:n]), bs
    big = cdata.synthetic_queries(md, 9000, seed=3)
    for off in (17, 3950):            # 3950 + 300 crosses the 4,096-query chunk
        be1, brel = torch.as_tensor(big["e1"]).clone(), torch.as_tensor(big["rel"]).clone()
        be1[off:off + 300] = e1
        brel[off:off + 300] = rel
        assert torch.equal(m.encode(be1, brel)[off:off + 300], h), off
    m.close()
    # ... and whatever the chunk: a handle planned with 128-query chunks gives the same bits
    monkeypatch.setenv("COPER_FACTORED_CHUNK", "128")
    m2 = _model(md, p)
    assert torch.equal(m2.encode(e1, rel), h)
    m2.close()


def test_ragged_and_hostile_inputs(oracle_chain):
    O = oracle_chain
    md = cdata.model_descriptors("nations_cpg", num_ent=300)
    p = cdata.synthetic_params(md, 2)
    m = _model(md, p)
    q = cdata.synthetic_queries(md, 130, seed=4)
    full = m.encode(q["e1"], q["rel"]).clone()
    st = O.forward(p, md, q["e1"], q["rel"], np.float64)
    assert np.abs(full.cpu().numpy() - st["h"]).max() < H_TOL
    for B in (0, 1, 15, 16, 17, 33, 130):
        h = m.encode(q["e1"][:B], q["rel"][:B])
        assert tuple(h.shape) == (B, md["ent_emb_size"])
        assert torch.equal(h, full[:B]), B
    m.encode(q["e1"], q["rel"])
    assert m.check_ids() == 0
    e1, rel = q["e1"].copy(), q["rel"].copy()
    rel[3], rel[77], e1[50] = md["num_rel"], -1, md["num_ent"] + 5
    h = m.encode(e1, rel)
    assert m.check_ids() == 3
    assert torch.isfinite(h).all()
    ok = np.ones(130, bool)
    ok[[3, 77, 50]] = False
    assert torch.equal(h[torch.as_tensor(ok)], full[torch.as_tensor(ok)])
    # clamped like the cached path: relation 0
    assert torch.equal(h[3], m.encode(e1[3:4], np.zeros(1, np.int64))[0])
    m.encode(q["e1"], q["rel"])
    assert m.check_ids() == 0
    # a relation that occurs once among another that fills the batch
    rel2 = np.full(130, 5, np.int64)
    rel2[64] = 9
    h2 = m.encode(q["e1"], rel2)
    st2 = O.forward(p, md, q["e1"], rel2, np.float64)
    assert np.abs(h2.cpu().numpy() - st2["h"]).max() < H_TOL
    m.close()


_TRAIN = dict(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=0.003)


def _train_batch(md, B, L, seed):
    rng = np.random.default_rng(seed)
    E, R = md["num_ent"], md["num_rel"]
    lookup = rng.integers(0, E, (B, L)).astype(np.int32)
    labels = np.zeros((B, L), np.float32)
    labels[:, 0] = 1.0
    return dict(e1=rng.integers(0, E, B), rel=rng.integers(0, R, B), lookup_values=lookup, e2_multi=labels)


@pytest.mark.parametrize("case", ["nations_cpg", "mlp300"])
def test_inference_after_training_steps(oracle_chain, case):
    from coper_amd.metrics import ranking_and_hits
    O = oracle_chain
    if case == "nations_cpg":
        md = cdata.model_descriptors("nations_cpg", **_TRAIN)
    else:
        md = cdata.model_descriptors("nations_cpg", num_ent=300, num_rel=12, context_rel_out=[12], context_rel_use_batch_norm=True, **_TRAIN)
    p0 = cdata.synthetic_params(md, seed=3)
    m = _model(md, {k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=0)
    for step in range(3):
        m.train_step(_train_batch(md, 48, 20, step))
    # the stale handle refuses a raw encode (the rule stays enforced); the wrapper prepares again by itself
    q = cdata.synthetic_queries(md, 200, seed=6)
    ids = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    out = torch.empty((4, md["ent_emb_size"]), device="cuda:0")
    rc = m._lib.coper_encode(m._h, C.c_void_p(ids.data_ptr()), C.c_void_p(ids.data_ptr()), 4, None, C.c_void_p(out.data_ptr()), None)
    assert rc == 5, rc                                          # COPER_ESTATE
    mr, mrr, hits, ranks = ranking_and_hits(m, None, cdata.EvalDataset(q, 64, md["num_ent"]), "after-step", return_ranks=True)
    pv = {k: v.detach().cpu().numpy().copy() for k, v in m._tensors.items()}       # the variables as the steps left them
    assert any(not np.array_equal(pv[k], np.asarray(p0[k], np.float32)) for k in pv)
    c = _model(md, pv, dense="cached")
    hf, hc = m.encode(q["e1"], q["rel"]), c.encode(q["e1"], q["rel"])
    st = O.forward(pv, md, q["e1"], q["rel"], np.float64)
    d_fc = float((hf - hc).abs().max())
    d_f, d_c = np.abs(hf.cpu().numpy() - st["h"]).max(), np.abs(hc.cpu().numpy() - st["h"]).max()
    print("%s after 3 steps: |h_fac - h_cached| = %.3e, |h_fac - f64| = %.3e, |h_cached - f64| = %.3e" % (case, d_fc, d_f, d_c))
    assert d_fc < H_TOL and d_f < H_TOL and d_c < H_TOL
    assert np.array_equal(_check_ranks_are_the_chains(O, m, hf, pv, q), ranks)
    _check_ranks_are_the_chains(O, c, hc, pv, q)
    m.close()
    c.close()


def test_no_cache_is_held():
    """FB15k-237 shapes: a factored handle after prepare() and one 2,048-query rank_pass holds less than ONE of the two 16-bit cache
    planes of a cached handle (R2 F d 2 bytes = 0.87 GB).  What it should hold: 118 MB P planes + ~60 MB entity images + <= 256 MB of
    T slices + ~75 MB x planes (a 4,096-query chunk; this pass allocates them for 2,048) ~ 0.5 GB."""
    from coper_amd import _lib
    lib = _lib.load()
    md = cdata.model_descriptors("fb15k237_cpg")
    p = cdata.synthetic_params(md, 0)
    q = cdata.synthetic_queries(md, 2048, seed=0)
    gc.collect()
    torch.cuda.synchronize()
    base = lib.coper_live_device_bytes()
    m = _model(md, p)
    m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
    torch.cuda.synchronize()
    held = lib.coper_live_device_bytes() - base
    F, d, R2 = m.fc_input_size, md["ent_emb_size"], md["num_rel"]
    print("factored handle at FB15k-237 shapes holds %.1f MB (one cache plane: %.1f MB)" % (held / 1e6, R2 * F * d * 2 / 1e6))
    assert 0 < held < R2 * F * d * 2
    m.close()
    assert lib.coper_live_device_bytes() == base


def test_drop_ins(golden_dir, oracle_chain):
    from coper_amd.fact_network import FactNetworkScorer
    from coper_amd.stream import RankStream
    _, md, p, q = _fwd_case(golden_dir, "cpg_fc")
    m = _model(md, p)
    h = m.encode(q["e1"], q["rel"])
    logits = m.score_all(h)
    sess = m.session()
    batch = dict(q, lookup_values=np.zeros((len(q["e1"]), 0), np.int32))
    e1f, predf, embf = sess.run((m.e1, m.predictions_all, m.predicted_e2_emb), {m.input_iterator_handle: [batch]})
    assert np.array_equal(predf, logits.cpu().numpy()) and np.array_equal(embf, h.cpu().numpy()) and np.array_equal(e1f, q["e1"])
    # RankStream over four batches (staged ids, ranks posted beside the next pass) == rank_pass on each
    B = len(q["e1"]) // 4
    batches, want = [], []
    for i in range(4):
        s, e = i * B, (i + 1) * B
        ip = q["filt_indptr"][s:e + 1]
        b = dict(e1=q["e1"][s:e], rel=q["rel"][s:e], e2=q["e2"][s:e], filt_indptr=ip - ip[0], filt_idx=q["filt_idx"][ip[0]:ip[-1]])
        batches.append(b)
        want.append(m.rank_pass(b["e1"], b["rel"], b["e2"], b["filt_indptr"], b["filt_idx"])[0].cpu().numpy())
    rs = RankStream(m, B, max(len(b["filt_idx"]) for b in batches))
    got = rs.run(batches)
    assert len(got) == 4 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert rs.stale_passes == 0
    m.close()
    g = np.load(os.path.join(golden_dir, "minerva_e2e.npz"))
    tag = "cpg"
    E, R, Bq, d1, d2, Cc, r_dim = (int(v) for v in g[tag + ":dims"])
    sd = {k.split(":sd:")[1]: torch.as_tensor(g[k]) for k in g.files if k.startswith(tag + ":sd:")}
    fn = FactNetworkScorer(sd, torch.as_tensor(g[tag + ":ent"]), g[tag + ":rel"], d1, d2, cpg=True, device="cuda:0", dense="factored")
    assert fn.model.dense == "factored"
    e1, r, e2 = (torch.as_tensor(g[tag + ":" + k].astype(np.int64)) for k in ("e1", "r", "e2"))
    S, Sf = fn.forward(e1, r), fn.forward_fact(e1, r, e2)
    assert tuple(S.shape) == (Bq, E) and tuple(Sf.shape) == (Bq, 1)
    assert np.abs(S.cpu().numpy() - g[tag + ":S"]).max() < 1e-4 and np.abs(Sf.cpu().numpy() - g[tag + ":S_fact"]).max() < 1e-4
    fn.close()


def test_capture_is_refused():
    from coper_amd import _lib
    md = cdata.model_descriptors("nations_cpg")
    p = cdata.synthetic_params(md, 0)
    q = cdata.synthetic_queries(md, 64, seed=0)
    m = _model(md, p)
    before = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])[0].clone()
    with pytest.raises(_lib.CoperError) as ei:
        m.capture_rank_pass(64, int(len(q["filt_idx"])))
    assert ei.value.code == EUNSUPPORTED
    after = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])[0]
    assert torch.equal(before, after)
    m.close()
