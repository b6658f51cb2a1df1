"""Entity embeddings wider than 320 (coper_create: ent_emb_size <= 640).  Beyond 320 the fragments of a 128-query tile no longer
fit the CU's 160 KiB of LDS; the count kernels of both score modes then hold the tile in two halves of K
(kernels_score3_wide_bf16.hip, k_score_count_wide_f32).  Everything else on the path is the code every other size takes, which no
size above 320 had run before: these tests take every public route of a handle through d = 324, 400, 512 and 640.

Tolerances are the project's (tests/test_gpu_fuzz.py, tests/test_gpu_scale.py, tests/test_gpu_train.py), not new numbers."""
import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from tests.helpers import rank_defining_logits

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3
H_TOL = 2e-4
AUDIT_BAR = 0.5
DEV = "cuda:0"

WIDE = {324: (18, 18), 400: (20, 20), 512: (16, 32), 640: (20, 32)}
VARIANTS = ["cpg_fc", "cpg_conv_fc", "cpg_mlp", "lookup", "plain", "cpg_fc_concat"]
ENTS = [5, 257, 700, 4099]
QS = [1, 63, 64, 65, 129, 520]      # both sides of a 64-query boundary and of the 128-query tile


def _md(d, variant="cpg_fc", num_ent=700, num_rel=6, C=8, r=8):
    emb_h, emb_w = WIDE[d] if d in WIDE else d
    md = dict(cdata._COMMON)
    md.update(num_ent=num_ent, num_rel=num_rel, ent_emb_size=emb_h * emb_w, rel_emb_size=r, emb_h=emb_h, emb_w=emb_w,
              conv_filter_height=3, conv_filter_width=3, conv_num_channels=C)
    if variant == "cpg_fc":
        md.update(context_rel_conv=None, context_rel_out=[])
    elif variant == "cpg_conv_fc":
        md.update(context_rel_conv=[], context_rel_out=[])
    elif variant == "cpg_mlp":
        md.update(context_rel_conv=[5], context_rel_out=[7, 6])
    elif variant == "lookup":
        md.update(context_rel_conv=[], context_rel_out=[], do_parameter_lookup=True)
    elif variant == "plain":
        md.update(context_rel_conv=None, context_rel_out=None, rel_emb_size=emb_h * emb_w)
    elif variant == "cpg_fc_concat":
        md.update(context_rel_conv=None, context_rel_out=[], concat_rel=True)
    else:
        raise KeyError(variant)
    return md


def _model(md, p, **kw):
    from coper_amd.models import ConvE
    if kw.get("score_mode") == "bf16x3":
        kw.setdefault("band_audit_period", 1)
    return ConvE(md, device=DEV, **kw).load_parameters(p).prepare()


def _closed_form(xl, q, E):
    Q = len(q["e2"])
    mask = cdata.csr_to_dense_filter(q["filt_indptr"], q["filt_idx"], E).astype(bool)
    tgt = xl[np.arange(Q), q["e2"]]
    keep = ~mask
    keep[np.arange(Q), q["e2"]] = False
    return 1 + ((xl > tgt[:, None]) & keep).sum(axis=1), ((xl == tgt[:, None]) & keep).sum(axis=1), keep


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the sizes construct, prepare and rank; the new bound is enforced
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("d", sorted(WIDE))
def test_wide_sizes_construct_prepare_and_rank(d, mode):
    from coper_amd.models import ConvE
    md = _md(d, num_ent=300)
    p = cdata.synthetic_params(md, seed=d)
    q = cdata.synthetic_queries(md, 70, seed=1)
    m = ConvE(md, device=DEV, score_mode=mode)
    m.load_parameters(p)
    m.prepare()
    ranks, ne = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
    r = ranks.cpu().numpy()
    assert r.shape == (70,) and (r >= 1).all() and (r <= md["num_ent"]).all()
    m.close()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_sizes_beyond_640_are_refused(mode):
    from coper_amd import _lib
    from coper_amd.models import ConvE
    md = _md((16, 41), num_ent=300)
    assert md["ent_emb_size"] == 656
    with pytest.raises(_lib.CoperError) as ei:
        m = ConvE(md, device=DEV, score_mode=mode)
        m.load_parameters(cdata.synthetic_params(md, seed=0))
        m.prepare()
    assert ei.value.code == 1, ei.value        # COPER_EINVAL
    assert "640" in str(ei.value), ei.value


# ---------------------------------------------------------------------------------------------------------------------------
# 2. parity per size and mode, in the manner of test_random_shapes_against_oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _parity_cases():
    out = []
    i = 0
    for d in sorted(WIDE):
        for variant in VARIANTS:
            # every |E| and every Q at every size: the pairs rotate so that six variants cover both lists
            out.append((d, variant, ENTS[(i + i // 4) % 4], QS[i % 6]))
            i += 1
    # the production channel count (C = 32: the dense layer of a wide handle runs on the fallback encoders with F = 18 x 18 x 32) and
    # a size that is no multiple of 4 (17 x 19 = 323, KS16 = 21: the scalar branches of the finalize, the packing and the chains)
    out.append((400, "cpg_fc", 700, 129, 32))
    out.append((512, "plain", 257, 65, 32))
    out.append(((17, 19), "cpg_fc", 700, 129, 8))
    out.append(((17, 19), "plain", 257, 520, 8))
    out.append(((17, 19), "lookup", 4099, 63, 32))
    return [c if len(c) == 5 else c + (8,) for c in out]


@pytest.mark.parametrize("d,variant,E,Q,C", _parity_cases())
def test_wide_shapes_against_oracle(oracle_chain, d, variant, E, Q, C):
    O = oracle_chain
    md = _md(d, variant, num_ent=E, C=C)
    d = md["ent_emb_size"]
    p = cdata.synthetic_params(md, seed=d + Q)
    q = cdata.synthetic_queries(md, Q, seed=E)
    st = O.forward(p, md, q["e1"], q["rel"], np.float64, materialise=False)
    ref_logits = O.score_all(st["h"], p["ent_emb"].astype(np.float64), p["pred_bias"].astype(np.float64))
    m32 = None
    for mode in ("f32", "bf16x3"):
        what = (d, variant, E, Q, C, mode)
        m = _model(md, p, score_mode=mode)
        h = m.encode(q["e1"], q["rel"])
        assert np.abs(h.cpu().numpy() - st["h"]).max() < H_TOL, what
        logits = m.score_all(h).cpu().numpy()
        assert np.abs(logits - ref_logits).max() < LOGIT_TOL, what
        if mode == "f32":       # the mode's logits ARE the chain: bit for bit against the C restatement on a 24-query sample
            sel = np.unique(np.linspace(0, Q - 1, min(Q, 24)).astype(np.int64))
            chain = O.score_chain(np.ascontiguousarray(h.cpu().numpy()[sel]), np.ascontiguousarray(p["ent_emb"], np.float32),
                                  np.ascontiguousarray(p["pred_bias"], np.float32))
            assert np.array_equal(logits[sel], chain), what
        # fused and two-call ranks and tie counts: the closed form on the library's own chain logits, every query
        xl = rank_defining_logits(O, m, h, p)
        want, want_eq, keep = _closed_form(xl, q, E)
        m.band_audit()
        ranks, ne = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
        assert np.array_equal(ranks.cpu().numpy(), want), what
        assert np.array_equal(ne.cpu().numpy(), want_eq), what
        r0, _ = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], want_equal=False)
        assert np.array_equal(r0.cpu().numpy(), want), what
        r2, ne2 = m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
        assert np.array_equal(r2.cpu().numpy(), want), what
        assert np.array_equal(ne2.cpu().numpy(), want_eq), what
        if mode == "bf16x3":
            ratio, n_pairs = m.band_audit()
            print("wide d=%d %s |E|=%d Q=%d: band audit %.3f over %d pairs" % (d, variant, E, Q, ratio, n_pairs))
            assert n_pairs > 0 and ratio < AUDIT_BAR, (what, ratio, n_pairs)
        # the pruned top-k: a stable sort of the masked rows of the mode's own logits
        masked = np.where(keep | (np.arange(E)[None, :] == q["e2"][:, None]), logits, -np.inf)
        order_all = np.lexsort((np.broadcast_to(np.arange(E), masked.shape), -masked), axis=1)
        tgt = m.target_scores(h, q["e2"])
        for k in (1, 10, 128):
            k = min(k, E)
            out = m.rank_counts(h, tgt, q["e2"], q["filt_indptr"], q["filt_idx"], k=k)
            order = order_all[:, :k]
            want_val = np.take_along_axis(masked, order, axis=1)
            got_val, got_idx = out[2].cpu().numpy(), out[3].cpu().numpy()
            assert np.array_equal(got_val, want_val), (what, k)
            fin = np.isfinite(want_val)
            assert np.array_equal(got_idx[fin], order[fin]), (what, k)
            assert np.array_equal(1 + out[0].cpu().numpy(), want), (what, k)
        # predict_topk: exact in both modes -- values, set and order of the fp32 chain's filtered rows (no entity exempt)
        if mode == "f32":
            m32 = m
        pm = np.where(cdata.csr_to_dense_filter(q["filt_indptr"], q["filt_idx"], E).astype(bool), -np.inf, m32.score_all(h).cpu().numpy())
        p_order = np.lexsort((np.broadcast_to(np.arange(E), pm.shape), -pm), axis=1)
        for k in (1, 10, 128):
            k = min(k, E)
            tv, ti = m.predict_topk(None, None, k, q["filt_indptr"], q["filt_idx"], h=h)
            wv = np.take_along_axis(pm, p_order[:, :k], axis=1)
            assert np.array_equal(tv.cpu().numpy(), wv), (what, k)
            fin = np.isfinite(wv)
            assert np.array_equal(ti.cpu().numpy()[fin], p_order[:, :k][fin]), (what, k)
            assert (ti.cpu().numpy()[~fin] == -1).all(), (what, k)
        if mode != "f32":
            m.close()
    m32.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. full-size parity: FB15k-237's shape at d = 512
# ---------------------------------------------------------------------------------------------------------------------------
def test_full_size_x3_equals_f32_and_the_c_closed_form(oracle_chain):
    from tests.test_gpu_scale import _pin_to_c_chain
    md = cdata.model_descriptors("fb15k237_cpg", ent_emb_size=512, emb_h=16, emb_w=32, conv_num_channels=8)
    p = cdata.synthetic_params(md, 0)
    Q = 20480
    q = cdata.synthetic_queries(md, Q, seed=0)
    m3 = _model(md, p, score_mode="bf16x3")
    m32 = _model(md, p, score_mode="f32")
    h = m3.encode(q["e1"], q["rel"])
    m3.band_audit()
    r3, ne3 = m3.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    ratio, n_pairs = m3.band_audit()
    r32, ne32 = m32.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    print("full size d=512: band audit %.3f over %d pairs" % (ratio, n_pairs))
    assert torch.equal(r3, r32) and torch.equal(ne3, ne32)
    assert n_pairs > 0 and ratio < AUDIT_BAR, (ratio, n_pairs)
    rf, nef = m3.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
    assert torch.equal(rf, r32) and torch.equal(nef, ne32)
    _pin_to_c_chain(oracle_chain, p, h, q, lambda sel: m32.score_all(h[torch.as_tensor(sel, device=h.device)].contiguous()).cpu().numpy(),
                    r32, ne32)
    m3.close()
    m32.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. operand scales at d = 512 (the scenarios of tests/test_gpu_scale.py that do not need its full size)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["xavier", "n1e-2", "n1e-3", "tiny", "rowspread", "clamp"])
def test_x3_ranks_equal_chain_at_every_table_scale_d512(kind, oracle_chain):
    from tests.test_gpu_scale import _check, _tables
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=4099, num_rel=40, ent_emb_size=512, emb_h=16, emb_w=32, conv_num_channels=8)
    p = _tables(kind, md, 0)
    rel, ratio, n = _check(md, p, 1024, O=oracle_chain)
    print("d=512 %-10s max |s_x3 - s_chain| = %.3f of the band's allowance; band audit %.3f over %d pairs" % (kind, rel, ratio, n))


@pytest.mark.parametrize("d", [400, 640])
def test_band_audit_at_the_other_sizes(d, oracle_chain):
    """The audit ratio DESIGN 4.3 records for d = 400 and 640 (d = 512: the test above), on the tables the reference starts from
    and on N(0, 1e-2) tables."""
    from tests.test_gpu_scale import _check, _tables
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=4099, num_rel=40, ent_emb_size=d, emb_h=WIDE[d][0], emb_w=WIDE[d][1],
                                 conv_num_channels=8)
    for kind in ("xavier", "n1e-2"):
        rel, ratio, n = _check(md, _tables(kind, md, 0), 1024, O=oracle_chain)
        print("d=%d %-10s max |s_x3 - s_chain| = %.3f of the band's allowance; band audit %.3f over %d pairs" % (d, kind, rel, ratio, n))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the other paths at d = 400
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("bounds", [[(0, 333), (333, 700)], [(0, 100), (100, 421), (421, 700)]])
def test_entity_shards_sum_to_the_unsharded_result(bounds, mode):
    from coper_amd.sharding import merge_topk
    md = _md(400, num_ent=700)
    p = cdata.synthetic_params(md, seed=4)
    q = cdata.synthetic_queries(md, 200, seed=4)
    full = _model(md, p, score_mode=mode)
    h = full.encode(q["e1"], q["rel"])
    tgt_full = full.target_scores(h, q["e2"])
    k = 10
    ng_f, ne_f, tv_f, ti_f = full.rank_counts(h, tgt_full, q["e2"], q["filt_indptr"], q["filt_idx"], k=k)
    shards = [_model(md, p, score_mode=mode, shard=b) for b in bounds]
    rows = sum(s.gather_entities(q["e1"]) for s in shards)
    assert np.array_equal(rows.cpu().numpy(), np.asarray(p["ent_emb"], np.float32)[q["e1"]])
    hs = shards[-1].encode(q["e1"], q["rel"], e1_rows=rows)
    assert torch.equal(hs, h)
    tgt = sum(s.target_scores(hs, q["e2"]) for s in shards)
    assert torch.equal(tgt, tgt_full)
    outs = [s.rank_counts(hs, tgt, q["e2"], q["filt_indptr"], q["filt_idx"], k=k) for s in shards]
    assert torch.equal(sum(o[0] for o in outs), ng_f) and torch.equal(sum(o[1] for o in outs), ne_f)
    tv, ti = merge_topk(torch.cat([o[2] for o in outs], dim=1), torch.cat([o[3] for o in outs], dim=1), k)
    assert torch.equal(tv, tv_f)
    fin = torch.isfinite(tv_f)
    assert torch.equal(ti[fin], ti_f[fin])
    # the packed exchange of step 1 carries d + 1 columns
    local = torch.arange(0, min(50, bounds[0][1]), dtype=torch.int64, device=DEV)
    buf = shards[0].pack_owned_rows(local, 64, 1.0, 2.0)
    assert buf.shape == (65, 401)
    for s in shards + [full]:
        s.close()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_graph_replay_equals_the_eager_pass(mode):
    md = _md(400, num_ent=700)
    p = cdata.synthetic_params(md, seed=6)
    m = _model(md, p, score_mode=mode)
    B = 256
    q = cdata.synthetic_queries(md, B, seed=6)
    run = m.capture_rank_pass(B, int(q["filt_idx"].size) + 64)
    for seed in (6, 7):
        q = cdata.synthetic_queries(md, B, seed=seed)
        if q["filt_idx"].size > int(cdata.synthetic_queries(md, B, seed=6)["filt_idx"].size) + 64:
            continue
        r_e, ne_e = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
        r_e, ne_e = r_e.clone(), ne_e.clone()
        r_g, ne_g = run(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
        assert torch.equal(r_g, r_e) and torch.equal(ne_g, ne_e), (mode, seed)
    del run
    m.close()


def test_factored_handle_against_the_oracle(oracle_chain):
    O = oracle_chain
    md = _md(400, "cpg_fc", num_ent=700)
    p = cdata.synthetic_params(md, seed=8)
    q = cdata.synthetic_queries(md, 300, seed=8)
    st = O.forward(p, md, q["e1"], q["rel"], np.float64, materialise=False)
    ref_logits = O.score_all(st["h"], p["ent_emb"].astype(np.float64), p["pred_bias"].astype(np.float64))
    m = _model(md, p, score_mode="bf16x3", dense="factored")
    h = m.encode(q["e1"], q["rel"])
    assert np.abs(h.cpu().numpy() - st["h"]).max() < H_TOL
    assert np.abs(m.score_all(h).cpu().numpy() - ref_logits).max() < LOGIT_TOL
    xl = rank_defining_logits(O, m, h, p)
    want, want_eq, _ = _closed_form(xl, q, md["num_ent"])
    r, ne, h2 = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], want_h=True)
    xl2 = rank_defining_logits(O, m, h2, p)
    want2, want_eq2, _ = _closed_form(xl2, q, md["num_ent"])
    assert np.array_equal(r.cpu().numpy(), want2) and np.array_equal(ne.cpu().numpy(), want_eq2)
    r2, ne2 = m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    assert np.array_equal(r2.cpu().numpy(), want) and np.array_equal(ne2.cpu().numpy(), want_eq)
    m.close()


_TRAIN_D400 = {
    "cpg_linear": dict(num_ent=211, num_rel=6, ent_emb_size=400, rel_emb_size=8, emb_h=20, emb_w=20, conv_num_channels=8,
                       context_rel_conv=None, context_rel_out=[]),
    "plain": dict(num_ent=211, num_rel=6, ent_emb_size=400, rel_emb_size=400, emb_h=20, emb_w=20, conv_num_channels=8,
                  context_rel_conv=None, context_rel_out=None),
    # d % 4 != 0 beyond 320: the scalar (non-vector) branches of the step
    "cpg_linear_d323": dict(num_ent=211, num_rel=6, ent_emb_size=323, rel_emb_size=8, emb_h=17, emb_w=19, conv_num_channels=8,
                            context_rel_conv=None, context_rel_out=[]),
}


@pytest.mark.parametrize("one_vs_all", [False, True])
@pytest.mark.parametrize("name", sorted(_TRAIN_D400))
def test_train_step_matches_oracle_at_d400(name, one_vs_all):
    """Two steps against the float64 training oracle, each from the device's variables (the step-0 bounds of tests/test_gpu_train.py)."""
    from tests.test_gpu_train import _train_step_case
    _train_step_case(name, True, one_vs_all, "n0.1", steps=2, case=_TRAIN_D400[name])
