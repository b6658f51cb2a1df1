"""The filter correction read from the count kernel's own compare bits (kernels_score3_bf16.hip: the gt plane and the look-up role of
the band launch; kernels_tail_bf16.hip: the tail kernel without filter tiles).

A ranks-only `rank_pass` of the bf16x3 mode on a handle the fused tail serves (13 or 16 k-steps, the whole table) no longer scores
its known answers a second time: the count launch stores one bit per logit "above the band" and the band launch takes the set bits of
the filter entries back from the ranks.  What can go wrong is the ADDRESS of a bit -- (tile, row of a wave, lane, word, bit) from
(query, entity) -- and the rule for which entries count, so the shapes here are chosen for the addressing, not for the workload:
|E| with a partial last row of 512 entities and one entity past a row, Q with a partial 128-query tile and a partial 16-column
block, d with the half tail, the full tail and no tail of the x3 logit.  The reference of every case is the fp32-exact mode ranking
the SAME h (what the bf16x3 mode's ranks are defined as), bit for bit."""
import os

import numpy as np
import pytest
import torch

from coper_amd import data as cdata

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = {200: (10, 20), 208: (13, 16), 256: (16, 16)}      # half tail, full tail, no tail
ES = (14, 257, 513, 1000, 4099)
QS = (1, 33, 129, 300)
E_MAX = max(ES)


def _own_entries():
    """TL_OWN_ENTRIES of this build (tail_tile.h): 32 entries per tile, COPER_TL_OWN_TILES = 3 * COPER_TL_WAVES - 1 tiles -- the share of
    a 32-query block the old tail kernel takes back itself, beyond which a block is `heavy`."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "coper_amd", "csrc", "tail_tile.h")).read()
    waves = int(re.search(r"#define COPER_TL_WAVES (\d+)", src).group(1))
    assert "#define COPER_TL_OWN_TILES (3 * COPER_TL_WAVES - 1)" in src and "TL_OWN_ENTRIES = 32 * (int64_t)(COPER_TL_OWN_TILES)" in src
    return 32 * (3 * waves - 1)


OWN_ENTRIES = _own_entries()
LOOKUP_OWN = 256             # BL_OWN: entries of its 16 queries a wave of the look-up role takes itself (kernels_score3_bf16.hip)


def _md(E, d, **kw):
    return cdata.model_descriptors("fb15k237_cpg", **dict(dict(num_ent=E, num_rel=14, ent_emb_size=d, emb_h=GRID[d][0], emb_w=GRID[d][1],
                                                               rel_emb_size=8), **kw))


def _model(md, p, mode="bf16x3", **kw):
    from coper_amd.models import ConvE
    return ConvE(md, device=DEV, score_mode=mode, **kw).load_parameters(p).prepare()


@pytest.fixture(scope="module")
def params_of():
    """d -> the parameters of the largest table (built once; smaller tables take its first rows)."""
    cache = {}

    def get(d, E):
        if d not in cache:
            cache[d] = cdata.synthetic_params(_md(E_MAX, d), 5)
        return {k: (v[:E] if k in ("ent_emb", "pred_bias") else v) for k, v in cache[d].items()}

    yield get
    cache.clear()


def _csr(rows):
    ip = np.zeros(len(rows) + 1, np.int64)
    ip[1:] = np.cumsum([len(r) for r in rows])
    return ip, (np.concatenate(rows).astype(np.int64) if len(rows) else np.zeros(0, np.int64))


def _rows_of_every_kind(E, e2, rng):
    """One filter row per query, the kinds dealt in turn (rows ascending, as the loaders give them):
    0 a synthetic row (the target and a few random entities); 1 EVERY entity; 2 empty; 3 only the target; 4 adjacent duplicates and an
    entry equal to the target; 5 a row longer than a whole 32-query block's old own share (the old heavy case)."""
    rows, kinds = [], []
    for i, t in enumerate(e2):
        k = i % 6 if i < 24 else 0          # (the long kinds on the first queries only: the case stays small)
        if k == 0:
            r = np.unique(np.concatenate([rng.integers(0, E, int(rng.integers(0, 12))), [t]]))
        elif k == 1:
            r = np.arange(E)
        elif k == 2:
            r = np.zeros(0, np.int64)
        elif k == 3:
            r = np.array([t])
        elif k == 4:
            r = np.sort(np.repeat(np.unique(np.concatenate([rng.integers(0, E, 9), [t]])), 3))
        else:
            u = np.unique(rng.integers(0, E, 400))
            r = np.sort(np.repeat(u, -(-(OWN_ENTRIES + 40) // len(u))))
            assert len(r) > OWN_ENTRIES > LOOKUP_OWN
        rows.append(r.astype(np.int64))
        kinds.append(k)
    return rows, np.array(kinds)


def _fused(m, q, ip, ix, want_h=False):
    m.profile(True)
    m.profile_read("tail"); m.profile_read("band_lookup"); m.profile_read("band_exact")
    out = m.rank_pass(q["e1"], q["rel"], q["e2"], ip, ix, want_equal=False, want_h=want_h)
    torch.cuda.synchronize()
    n_tail, n_look, n_band = m.profile_read("tail")[1], m.profile_read("band_lookup")[1], m.profile_read("band_exact")[1]
    m.profile(False)
    return out, (n_tail, n_look, n_band)


@pytest.mark.parametrize("d", sorted(GRID))
@pytest.mark.parametrize("E", ES)
def test_ranks_are_the_fp32_chains_on_every_bit_position(params_of, E, d):
    """Every (|E|, d) with every Q: rows of every kind.  The ranks are those of an f32-mode handle ranking the same h; a query whose
    row lists every entity has rank 1; the band launch carried the look-up role."""
    md = _md(E, d)
    p = params_of(d, E)
    m, m32 = _model(md, p), _model(md, p, "f32")
    rng = np.random.default_rng(1000 * E + d)
    for Q in QS:
        q = cdata.synthetic_queries(md, Q, seed=Q)
        rows, kinds = _rows_of_every_kind(E, q["e2"], rng)
        ip, ix = _csr(rows)
        (r, none, h), (n_tail, n_look, n_band) = _fused(m, q, ip, ix, want_h=True)
        assert none is None and n_tail == 1 and n_look == n_band == 1, (n_tail, n_look, n_band)
        r = r.cpu().numpy()
        want, _ = m32.rank(h, q["e2"], ip, ix)
        assert np.array_equal(r, want.cpu().numpy()), (E, d, Q, np.nonzero(r != want.cpu().numpy())[0][:8])
        assert (r[kinds == 1] == 1).all()
        assert (r >= 1).all() and (r <= E).all()
    m.close(); m32.close()


@pytest.mark.parametrize("d", sorted(GRID))
def test_planted_targets_few_above_some_inside_the_band(params_of, d):
    """Targets among the top few logits of the f32 handle's row, on a table whose odd rows repeat their even neighbours: the target's
    twin scores the target's logit exactly -- a known answer INSIDE the band, which is no gt bit and which the band walk passes over --
    and the known answers above are few.  Ranks of the f32 handle on the same h."""
    E, Q = 1000, 300
    md = _md(E, d)
    p = dict(params_of(d, E))
    p["ent_emb"] = np.repeat(p["ent_emb"][0::2], 2, axis=0).copy()
    p["pred_bias"] = np.repeat(p["pred_bias"][0::2], 2).copy()
    m, m32 = _model(md, p), _model(md, p, "f32")
    q = cdata.synthetic_queries(md, Q, seed=3)
    h = m.encode(q["e1"], q["rel"])
    top = torch.topk(m32.score_all(h), 12, dim=1).indices.cpu().numpy()
    rng = np.random.default_rng(d)
    e2 = top[np.arange(Q), rng.integers(0, 8, Q)]
    rows = []
    for i in range(Q):
        known = top[i, rng.random(12) < 0.4]
        rows.append(np.unique(np.concatenate([known, [e2[i], e2[i] ^ 1]])))       # the twin: inside the band
    ip, ix = _csr(rows)
    q = dict(q, e2=e2.astype(np.int64))
    (r, _), (n_tail, n_look, _) = _fused(m, q, ip, ix)
    assert n_tail == 1 and n_look == 1
    want, ne = m32.rank(h, q["e2"], ip, ix)
    assert np.array_equal(r.cpu().numpy(), want.cpu().numpy())
    # (the inputs are what they claim: some known answers were above the target, and no rank counts a known answer)
    r0, _ = m32.rank(h, q["e2"], np.zeros(Q + 1, np.int64), np.zeros(0, np.int64))
    assert (r0.cpu().numpy() > want.cpu().numpy()).sum() > Q // 4
    m.close(); m32.close()


def test_several_count_launches_in_one_pass(params_of, monkeypatch):
    """COPER_TOPK_CHUNK_QUERIES cuts the pass into count launches of 128 queries: each band launch looks up the entries of its own
    chunk, at the chunk's own bit addresses."""
    E, d, Q = 513, 200, 300
    md = _md(E, d)
    p = params_of(d, E)
    m, m32 = _model(md, p), _model(md, p, "f32")
    q = cdata.synthetic_queries(md, Q, seed=8)
    rows, kinds = _rows_of_every_kind(E, q["e2"], np.random.default_rng(8))
    rows = rows[::-1]                       # (the long rows in the LAST chunk)
    ip, ix = _csr(rows)
    (whole, _), _ = _fused(m, q, ip, ix)
    monkeypatch.setenv("COPER_TOPK_CHUNK_QUERIES", "128")
    (r, _, h), (n_tail, n_look, n_band) = _fused(m, q, ip, ix, want_h=True)
    assert n_tail == 1 and n_look == n_band == 3
    want, _ = m32.rank(h, q["e2"], ip, ix)
    assert np.array_equal(r.cpu().numpy(), want.cpu().numpy()) and torch.equal(r, whole)
    m.close(); m32.close()


def test_a_stale_grouping_still_returns_stale_everywhere(params_of):
    """The recipe of test_gpu_pipeline.py::test_the_guard_through_the_c_abi on a small batch: the tail kernel presets
    COPER_RANK_STALE, and what the count launch, the band walk and the look-up role add or subtract keeps every rank negative."""
    from coper_amd import _lib
    E, d, Q = 1000, 200, 300
    md = _md(E, d)
    m = _model(md, params_of(d, E))
    qa, qb = cdata.synthetic_queries(md, Q, seed=11), cdata.synthetic_queries(md, Q, seed=12)
    rows, _ = _rows_of_every_kind(E, qb["e2"], np.random.default_rng(12))
    qb["filt_indptr"], qb["filt_idx"] = _csr(rows)
    da = {k: torch.as_tensor(np.asarray(v)).to(DEV) for k, v in qa.items()}
    db = {k: torch.as_tensor(np.asarray(v)).to(DEV) for k, v in qb.items()}

    def pass_b():
        return m.rank_pass(db["e1"], db["rel"], db["e2"], db["filt_indptr"], db["filt_idx"], want_equal=False)[0].cpu().numpy()

    base = pass_b()
    assert (base >= 1).all() and m.stale_passes() == 0
    m.group_next(db["e1"], db["rel"])
    m.rank_pass(da["e1"], da["rel"], da["e2"], da["filt_indptr"], da["filt_idx"], want_equal=False)
    old = int(db["rel"][Q // 3])
    db["rel"][Q // 3] = (old + 1) % md["num_rel"]
    got = pass_b()
    assert (got < 0).all() and got.max() <= _lib.RANK_STALE + 10 ** 8, got[:4]
    assert m.stale_passes() == 1 and m.stale_passes() == 0
    db["rel"][Q // 3] = old
    assert np.array_equal(pass_b(), base)          # the pass after a stale one groups itself
    m.close()


def test_beyond_the_cap_and_sharded_handles_take_the_old_path_and_agree(params_of, monkeypatch):
    """A pass whose gt plane would exceed the cap (64 MiB: more than 2^29 logits in one count launch) keeps the tail kernel's own filter
    tiles; cut into launches of 4,096 queries the same pass takes the new path: the same ranks.  And an entity-sharded ranker (never
    the fused tail) on the same data as an unsharded handle on the new path."""
    from coper_amd.sharding import EntityShardedRanker
    d = 200
    E, Q = 32768, 16500                      # 16,512 padded queries x 32,768 entities = 2^29 + 2^22 bits
    md = _md(E, d)
    p = cdata.synthetic_params(md, 6)
    m = _model(md, p)
    q = cdata.synthetic_queries(md, Q, seed=2)
    (big, _), (n_tail, n_look, n_band) = _fused(m, q, q["filt_indptr"], q["filt_idx"])
    assert n_tail == 1 and n_look == 0 and n_band == 1          # the old path: the tail kernel scored the filter entries itself
    monkeypatch.setenv("COPER_TOPK_CHUNK_QUERIES", "4096")
    (cut, _), (n_tail, n_look, n_band) = _fused(m, q, q["filt_indptr"], q["filt_idx"])
    assert n_tail == 1 and n_look == n_band == 5
    assert torch.equal(big, cut)
    monkeypatch.delenv("COPER_TOPK_CHUNK_QUERIES")
    m.close()
    # sharded: one shard of the world-1 ranker (target scores + rank counts: the two-call kernels) against the new path
    md = _md(1000, d)
    p = params_of(d, 1000)
    m = _model(md, p)
    q = cdata.synthetic_queries(md, 300, seed=4)
    rows, _ = _rows_of_every_kind(1000, q["e2"], np.random.default_rng(4))
    ip, ix = _csr(rows)
    (new, _), (_, n_look, _) = _fused(m, q, ip, ix)
    assert n_look == 1
    er = EntityShardedRanker(m)
    r_sh, _ = er.rank(dict(e1=q["e1"], rel=q["rel"], e2=q["e2"], filt_indptr=ip, filt_idx=ix))
    assert np.array_equal(r_sh.cpu().numpy(), new.cpu().numpy())
    m.close()


def _identity_encoder(E, B, pred):
    """A model whose ENCODER returns h = I_B rows for rel = 0 .. B - 1, so that rank_pass sees the logits `pred` [B, E]: the conv
    stage's BN has gamma 0 and beta (1, 0, 0, ...) -- x is 1 on channel 0 and 0 elsewhere --, the generated dense weights are 0 on
    channel 0's features, the generated dense bias of relation j is e_j (rel_emb = I, projection = I), the dense BN is the identity
    (variance 1 - eps).  h[b, k] = relu(0 + [k == b]); the chain is fma(1, pred, 0) + zeros = pred exactly."""
    d, R, C = 200, 64, 8
    assert B <= R
    md = _md(E, d, num_rel=R, rel_emb_size=R, conv_num_channels=C)
    p = cdata.synthetic_params(md, 0)
    p["rel_emb"] = np.eye(R, dtype=np.float32)
    w = p["fc_weights/CPG/Projection0"].reshape(R, -1, d)
    w[:, 0::C, :] = 0.0                                       # features are (i, j, channel): channel 0
    p["fc_weights/CPG/Projection0"] = w.reshape(R, -1)
    p["fc_bias/CPG/Projection0"] = np.eye(R, d, dtype=np.float32)
    p["Conv1BN/gamma"] = np.zeros(C, np.float32)
    p["Conv1BN/beta"] = np.zeros(C, np.float32); p["Conv1BN/beta"][0] = 1.0
    p["FCBN/gamma"] = np.ones(d, np.float32); p["FCBN/beta"] = np.zeros(d, np.float32)
    p["FCBN/moving_mean"] = np.zeros(d, np.float32)
    p["FCBN/moving_variance"] = np.full(d, np.float32(1) - np.float32(1e-3), np.float32)
    p["ent_emb"] = np.zeros((E, d), np.float32)
    p["ent_emb"][:, :B] = pred.T
    p["pred_bias"] = np.zeros(E, np.float32)
    return md, p


@pytest.mark.parametrize("name", ["rank_E14", "rank_E257", "rank_E4099", "rank_ties"])
def test_reference_rankers_recorded_ranks_through_rank_pass(golden_dir, name):
    """rank_*.npz hold the outputs of the reference's own ranker on (pred, e2, filter); here they come out of rank_pass, whose
    filter correction is the look-up role."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    pred, e2 = g["pred"], g["e2"]
    B, E = pred.shape
    md, p = _identity_encoder(E, B, pred)
    m = _model(md, p)
    q = dict(e1=np.zeros(B, np.int64), rel=np.arange(B, dtype=np.int64), e2=e2.astype(np.int64))
    (r, _, h), (n_tail, n_look, _) = _fused(m, q, g["filt_indptr"], g["filt_idx"], want_h=True)
    assert n_tail == 1 and n_look == 1
    assert torch.equal(h, torch.eye(B, md["ent_emb_size"], device=DEV)), "the identity encoder is not the identity"
    want = g["closed_form_rank"] if "closed_form_rank" in g.files else 1 + g["n_greater"]
    assert np.array_equal(r.cpu().numpy(), want)
    m.close()
