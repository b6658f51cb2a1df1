"""Results that depend on a fact an EARLIER call left behind: the rest of the suite checks each kernel from a freshly loaded handle or
ranker; these run the same kernels against the same references after the sequence of calls a training-and-evaluation loop makes.

A. EntityShardedRanker.rank_stream with the host far ahead of the device: every chunk's plan travels through a ring of four pinned
   buffers, and a slot must not be rewritten before the copy that reads it has run.
B. Parameters edited between training steps and between inference passes: the registered tensors ARE the variables, so an in-place
   torch edit must reach the training step's packing scale and the prepared inference caches -- and a leaf registered again at
   another address must be read there by every launch, never where it was first registered.
C. coper_train_grad after an evaluation pass, an encode or a reserve: the looked-up dense table's absent rows are zeroed by the
   relation counts of the STEP, not by whatever batch was grouped since."""
import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from tests.test_gpu_train import _CASES, _batch, _rel_err, _train_step_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ A. the plan ring of rank_stream
_SLEEP = {}


def _busy_stream(ms=250.0):
    """Holds the current stream busy for about `ms` milliseconds (torch.cuda._sleep, sized once from event-timed probes: the
    faster of two, so that a probe run at a clock still ramping up does not shorten the later sleeps)."""
    if "cycles_per_ms" not in _SLEEP:
        probe, rates = 5_000_000, []
        for _ in range(2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(probe)
            b.record()
            b.synchronize()
            rates.append(probe / max(a.elapsed_time(b), 1e-3))
        _SLEEP["cycles_per_ms"] = max(rates)
    torch.cuda._sleep(int(ms * _SLEEP["cycles_per_ms"]))


def _chunks(md, n=10, B=512, seed=300):
    """n distinct chunks of B queries each: host ids (what the plans read), targets and CSR filters already on the device"""
    out = []
    for i in range(n):
        q = cdata.synthetic_queries(md, B, seed=seed + i)
        out.append(dict(e1=q["e1"], rel=q["rel"], e2=q["e2"], e2_dev=torch.as_tensor(q["e2"]).to(DEV),
                        filt_indptr=torch.as_tensor(q["filt_indptr"]).to(DEV), filt_idx=torch.as_tensor(q["filt_idx"]).to(DEV)))
    for i in range(n):
        for j in range(i):
            assert not np.array_equal(out[i]["rel"], out[j]["rel"]) and not np.array_equal(out[i]["e1"], out[j]["e1"])
    return out


def _stream_equals_separate(ranker, chunks, ms=250.0):
    """rank_stream at its DEFAULT window, started behind `ms` of device work, against rank() of each chunk on its own."""
    want = [tuple(t.cpu().numpy() for t in ranker.rank(c, k=10)) for c in chunks]
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t0.record()
    _busy_stream(ms)
    t1 = torch.cuda.Event(enable_timing=True)
    t1.record()
    for k in (0, 10):
        if k:
            _busy_stream(ms)
        got = list(ranker.rank_stream(chunks, k=k))
        torch.cuda.synchronize()
        assert len(got) == len(chunks)
        for i, (g, w) in enumerate(zip(got, want)):
            g = tuple(t.cpu().numpy() for t in g)
            assert len(g) == (4 if k else 2)
            assert np.array_equal(g[0], w[0]), ("ranks", k, i, int((g[0] != w[0]).sum()))
            assert np.array_equal(g[1], w[1]), ("n_equal", k, i)
            if k:
                assert np.array_equal(g[3], w[3]), ("top-k ids", i)
                assert np.array_equal(g[2].view(np.int32), w[2].view(np.int32)), ("top-k values", i)
    # (the stream really was held: tens of milliseconds, where the host enqueues all ten chunks in a few)
    assert t0.elapsed_time(t1) > 0.25 * ms
    return want


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_rank_stream_with_the_host_far_ahead_one_shard(mode):
    """World 1, no process group: each plan holds only the chunk's relations (rel_all)."""
    from coper_amd.models import ConvE
    from coper_amd.sharding import EntityShardedRanker
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=40)
    p = cdata.synthetic_params(md, 4)
    m = ConvE(md, device=DEV, score_mode=mode).load_parameters(p).prepare()
    er = EntityShardedRanker(m)
    assert er.world == 1 and not er.dist
    chunks = _chunks(md)
    want = _stream_equals_separate(er, chunks)
    for c, w in zip(chunks, want):       # (and the separate ranks are the unsharded model's)
        r, _ = m.rank_pass(c["e1"], c["rel"], c["e2"], c["filt_indptr"].cpu().numpy(), c["filt_idx"].cpu().numpy())
        assert np.array_equal(r.cpu().numpy(), w[0])
    m.close()


@pytest.mark.parametrize("G,g", [(2, 0), (4, 1)])
def test_rank_stream_with_the_host_far_ahead_emulated_ranks(G, g):
    """One rank's work of a G-rank job (emulate_world), split encoder on a handle of its own: take1 / take2 / sel / order / take come
    from the ring.  The other ranks' rows read as this rank's, so the values mean nothing against the oracle -- but they are
    deterministic: the stream must give what rank() gives for each chunk on the same ranker."""
    from coper_amd.models import ConvE
    from coper_amd.sharding import EntityShardedRanker, shard_bounds
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=40)
    lo, hi = shard_bounds(md["num_ent"], G, g)
    p = cdata.synthetic_params(md, 4)
    pg = {k: (v[lo:hi] if k in ("ent_emb", "pred_bias") else v) for k, v in p.items()}
    sc = ConvE(md, device=DEV, shard=(lo, hi), score_mode="bf16x3", role="score").load_parameters(pg, global_rows=False).prepare()
    enc = ConvE(md, device=DEV, shard=(lo, hi), score_mode="bf16x3", role="encode", rel_mod=(G, g)).load_parameters(pg, global_rows=False).prepare()
    er = EntityShardedRanker(sc, encoder=enc, emulate_world=(G, g))
    assert er.world == G and er.overlap
    chunks = _chunks(md)
    pl = er.plan(chunks[0])
    assert pl.split and set(pl.off) >= {"take1", "take2", "sel", "order", "take"}
    _stream_equals_separate(er, chunks)
    sc.close()
    enc.close()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_ranking_and_hits_through_the_sharded_ranker_behind_a_busy_stream(mode):
    from coper_amd.metrics import ranking_and_hits
    from coper_amd.models import ConvE
    from coper_amd.sharding import EntityShardedRanker
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=40)
    p = cdata.synthetic_params(md, 6)
    q = cdata.synthetic_queries(md, 512 * 10, seed=8)
    m = ConvE(md, device=DEV, score_mode=mode).load_parameters(p).prepare()
    want = ranking_and_hits(m, None, cdata.EvalDataset(q, 512, md["num_ent"]), "plain", return_ranks=True)[3]
    torch.cuda.synchronize()
    _busy_stream()
    got = ranking_and_hits(m, None, cdata.EvalDataset(q, 512, md["num_ent"]), "sharded", max_chunk=512, ranker=EntityShardedRanker(m),
                           return_ranks=True)[3]
    assert np.array_equal(got, want), int((got != want).sum())
    m.close()


# ------------------------------------------------------------------------------------------------ B. parameters changed in between
def _dense_leaf(md):
    ctx = md.get("context_rel_out", None)
    return "fc_weights" if ctx is None else "fc_weights/CPG/Projection%d" % len(ctx)


def _edit(how):
    def edit(m, ref):
        leaf = _dense_leaf(m.model_descriptors)
        if how == "load_parameters":           # the documented route: the values x 16, registered again
            m.load_parameters({leaf: m._tensors[leaf] * 16})
            ref[leaf] = ref[leaf] * 16
        else:                                  # in place: torch sees it (the tensor's version counter), nothing is registered again
            f = 16.0 if how == "mul16" else 2.0 ** -30
            with torch.no_grad():
                m._tensors[leaf].mul_(f)
            ref[leaf] = ref[leaf] * f
    return edit


@pytest.mark.parametrize("how", ["load_parameters", "mul16", "mul2^-30"])
@pytest.mark.parametrize("name", ["plain", "cpg_linear", "cpg_mlp_bn", "cpg_wide", "plain_wide"])
def test_train_step_after_the_dense_weights_changed(name, how):
    """Variants whose step packs the dense weights by the magnitude the last optimizer pass recorded: two steps, the dense weights
    changed, one more step -- held to the step-0 bounds against the float64 oracle restarted from the device's variables."""
    _train_step_case(name, True, False, "n0.1", steps=3, edit=_edit(how))


def test_train_step_after_the_moving_statistics_were_registered_elsewhere():
    """BN moving statistics are variables like the trainable leaves: registered at another address between two steps (a checkpoint
    loaded into fresh tensors), the next step updates the NEW tensors -- by what a twin handle that never registered anything again
    moves its own, to the bound _train_step_case holds a moving statistic to -- and leaves the old ones bit for bit alone."""
    from coper_amd.models import ConvE
    md = dict(cdata._COMMON)
    md.update(_CASES["cpg_mlp_bn"])
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=0.003)
    moved = ["Conv1BN/moving_mean", "FCBN/moving_variance", "fc_weights/CPG/Projection0/BatchNorm/moving_mean",
             "fc_weights/CPG/Projection0/BatchNorm/moving_variance"]
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    pair = []
    for _ in range(2):
        m = ConvE(md, device=DEV).load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
        m.train_init(seed=5)
        m.train_step(_batch(md, 48, 37, seed=100))
        pair.append(m)
    m, twin = pair
    torch.cuda.synchronize()
    old = {k: m._tensors[k] for k in moved}
    kept = {k: t.clone() for k, t in old.items()}
    m.load_parameters({k: t.clone() for k, t in old.items()})
    for k in moved:
        assert m._tensors[k].data_ptr() != old[k].data_ptr()
    for x in pair:
        x.train_step(_batch(md, 48, 37, seed=101))
    torch.cuda.synchronize()
    for k in moved:
        got, want = m._tensors[k].cpu().numpy(), twin._tensors[k].cpu().numpy()
        tol = 2e-5 + 1e-5 * np.abs(want).max()
        if k == "Conv1BN/moving_mean":       # (mean(conv) carries conv1_bias, whose steps under batch statistics are rounding noise)
            tol += float((m._tensors["conv1_bias"] - twin._tensors["conv1_bias"]).abs().max())
        assert np.abs(got - want).max() < tol, (k, np.abs(got - want).max(), tol)
        assert np.abs(got - kept[k].cpu().numpy()).max() > 0, k      # (the step did move it)
        assert _same(old[k], kept[k]), k
    m.close()
    twin.close()


def _edit_inference(T, ent=True):
    with torch.no_grad():
        if ent:
            T["ent_emb"][7].mul_(8.0)
            T["ent_emb"].mul_(2.0 ** -10)
        if "fc_weights" in T:
            T["fc_weights"].mul_(-3.0)
        else:
            T["fc_weights/CPG/Projection0"].mul_(-3.0)
        if "rel_emb" in T:                   # (g_lookup has none)
            T["rel_emb"].mul_(0.5).add_(0.01)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


_MOVED = {"cpg": ("fb15k237_cpg", {}),
          "cpg_hidden_bn": ("fb15k237_cpg", dict(context_rel_out=[64], context_rel_conv=[16])),
          "plain": ("fb15k237_plain", {}),
          "lookup": ("fb15k237_cpg", dict(do_parameter_lookup=True, context_rel_conv=[]))}
_MOVED_CASES = [(c, mode, "cached") for c in _MOVED for mode in ("f32", "bf16x3")] + [("cpg", "bf16x3", "factored")]


def _every_route(m, q, lookup):
    """name -> tensor of every inference route that reads a registered leaf at launch time"""
    h = m.encode(q["e1"], q["rel"])
    out = {"encode": h}
    out["rank"], out["rank n_equal"] = m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    out["rank_pass"], out["rank_pass n_equal"] = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
    out["score_all"] = m.score_all(h)
    out["score_lookup"] = m.score_lookup(h, lookup)
    out["target_scores"] = m.target_scores(h, q["e2"])
    out["gather_entities"] = m.gather_entities(q["e2"])
    out["predict_topk val"], out["predict_topk idx"] = m.predict_topk(q["e1"], q["rel"], 5, q["filt_indptr"], q["filt_idx"])
    return out


@pytest.mark.parametrize("case,mode,dense", _MOVED_CASES, ids=["-".join(c) for c in _MOVED_CASES])
def test_inference_after_every_parameter_was_registered_at_a_new_address(case, mode, dense):
    """encode + rank, then EVERY leaf registered again from an edited clone (a checkpoint loaded into fresh tensors) while the old
    tensors stay alive full of NaN: after prepare every inference route is a fresh model's of the same values, bit for bit, and free
    of NaN -- no launch site reads a pointer it kept from the first registration."""
    from coper_amd.models import ConvE
    name, over = _MOVED[case]
    md = cdata.model_descriptors(name, num_ent=3000, num_rel=40, **over)
    p = {k: torch.as_tensor(v).to(DEV) for k, v in cdata.synthetic_params(md, 9).items()}
    q = cdata.synthetic_queries(md, 300, seed=10)
    lookup = np.random.default_rng(3).integers(0, md["num_ent"], (300, 8)).astype(np.int32)
    m = ConvE(md, device=DEV, score_mode=mode, dense=dense).load_parameters(p).prepare()
    h0 = m.encode(q["e1"], q["rel"])
    m.rank(h0, q["e2"], q["filt_indptr"], q["filt_idx"])
    torch.cuda.synchronize()
    old = dict(m._tensors)
    assert set(old) == set(m.parameter_specs)
    clones = {k: t.clone() for k, t in old.items()}
    _edit_inference(clones)
    m.load_parameters(clones)
    for k, t in old.items():
        assert m._tensors[k].data_ptr() != t.data_ptr(), k
        t.fill_(float("nan"))          # (kept alive: the allocator cannot hand these addresses to the clones or to `fresh`)
    m.prepare()
    fresh = ConvE(md, device=DEV, score_mode=mode, dense=dense).load_parameters({k: t.clone() for k, t in clones.items()}).prepare()
    got, want = _every_route(m, q, lookup), _every_route(fresh, q, lookup)
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and (_same(g, w) if g.dtype == torch.float32 else torch.equal(g, w)), k
        assert not (g.dtype == torch.float32 and bool(torch.isnan(g).any())), k
    assert not _same(got["encode"], h0)
    assert all(bool(torch.isnan(t).all()) for t in old.values())
    m.close()
    fresh.close()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_inference_after_parameters_edited_in_place(mode):
    """encode + rank, then the registered tensors edited in place: the next encode, rank and score_all are a fresh model's of the
    edited tensors, bit for bit."""
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=40)
    p = {k: torch.as_tensor(v).to(DEV) for k, v in cdata.synthetic_params(md, 9).items()}
    q = cdata.synthetic_queries(md, 700, seed=10)
    m = ConvE(md, device=DEV, score_mode=mode).load_parameters(p).prepare()
    h0 = m.encode(q["e1"], q["rel"])
    r0, _ = m.rank(h0, q["e2"], q["filt_indptr"], q["filt_idx"])
    torch.cuda.synchronize()
    _edit_inference(m._tensors)
    fresh = ConvE(md, device=DEV, score_mode=mode).load_parameters({k: t.clone() for k, t in m._tensors.items()}).prepare()
    h1, hf = m.encode(q["e1"], q["rel"]), fresh.encode(q["e1"], q["rel"])
    assert _same(h1, hf) and not _same(h1, h0)
    r1, n1 = m.rank(h1, q["e2"], q["filt_indptr"], q["filt_idx"])
    rf, nf = fresh.rank(hf, q["e2"], q["filt_indptr"], q["filt_idx"])
    assert torch.equal(r1, rf) and torch.equal(n1, nf)
    assert _same(m.score_all(hf), fresh.score_all(hf))
    assert m.ent_absmax() == fresh.ent_absmax()
    m.close()
    fresh.close()


def test_inference_after_an_in_place_edit_two_shards_bf16x3():
    """Two shard handles of one table (bf16x3: one power of two for both shards' entity planes).  After an in-place edit of the
    table the shards re-agree on its maximum (what EntityShardedRanker does per chunk): their logits are those of fresh shards
    loaded with the edited table."""
    from coper_amd.models import ConvE
    from coper_amd.sharding import shard_bounds
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=40)
    P = {k: torch.as_tensor(v).to(DEV) for k, v in cdata.synthetic_params(md, 12).items()}
    bounds = [shard_bounds(md["num_ent"], 2, g) for g in range(2)]
    shards = [ConvE(md, device=DEV, shard=b, score_mode="bf16x3").load_parameters(P).prepare() for b in bounds]
    gen = torch.Generator(device=DEV).manual_seed(3)
    h = 0.3 * torch.randn((300, md["ent_emb_size"]), device=DEV, generator=gen)
    before = [s.score_all(h) for s in shards]
    assert len({s.ent_absmax() for s in shards}) == 2          # (each shard's own maximum, as a ranker reads it every chunk)
    torch.cuda.synchronize()
    with torch.no_grad():
        P["ent_emb"][bounds[1][0] + 5].mul_(8.0)            # a row of shard 1: the table's maximum moves there
        P["ent_emb"].mul_(2.0 ** -10)
    M = max(s.ent_absmax() for s in shards)
    for s in shards:
        s.set_x3_ent_absmax(M)
    E = P["ent_emb"].clone()
    assert M == float(E.abs().max())
    fresh = [ConvE(md, device=DEV, shard=b, score_mode="bf16x3").load_parameters({k: t.clone() for k, t in P.items()}).prepare() for b in bounds]
    for s, f, b0 in zip(shards, fresh, before):
        got = s.score_all(h)
        assert _same(got, f.score_all(h)) and not _same(got, b0)
    for x in shards + fresh:
        x.close()


def test_untouched_parameters_do_not_prepare_again(monkeypatch):
    """The check behind B costs nothing when nothing changed: back-to-back passes never call coper_prepare; one in-place edit,
    one prepare; parameters_changed() (writes torch does not see) one more."""
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=3000, num_rel=40)
    p = {k: torch.as_tensor(v).to(DEV) for k, v in cdata.synthetic_params(md, 1).items()}
    q = cdata.synthetic_queries(md, 256, seed=2)
    m = ConvE(md, device=DEV, score_mode="bf16x3").load_parameters(p).prepare()
    calls = []
    real = m._lib.coper_prepare

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(m._lib, "coper_prepare", counted)
    for _ in range(20):
        h = m.encode(q["e1"], q["rel"])
        m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
        m.score_all(h[:4])
        m.ent_absmax()
    assert len(calls) == 0
    with torch.no_grad():
        m._tensors["pred_bias"].add_(0.5)
    h = m.encode(q["e1"], q["rel"])
    m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    assert len(calls) == 1
    m.parameters_changed("pred_bias")
    m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    assert len(calls) == 2
    torch.cuda.synchronize()
    m.close()


# ------------------------------------------------------------------------------------------------ C. train_grad after other calls
_LOOKUP = {"lookup_r12": dict(_CASES["lookup"], num_rel=12)}


@pytest.mark.parametrize("name", ["lookup", "lookup_conv", "lookup_narrow_F", "lookup_r12"])
def test_train_grad_after_an_evaluation_pass(name):
    """A step on a batch that holds a strict subset of the relations, its gradients read; then, on the same handle, an evaluation
    pass on the complementary relations, an encode, a reserve that regrows the grouping workspace: the gradients read again are the
    same bits, and fc_weights (the looked-up table, whose absent rows are handed out as zeros) still the float64 oracle's."""
    from coper_amd.models import ConvE
    from oracle import coper_train_oracle as T
    md = dict(cdata._COMMON)
    md.update(_LOOKUP.get(name) or _CASES[name])
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=0.003)
    R, E, B, seed = md["num_rel"], md["num_ent"], 48, 5
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = ConvE(md, device=DEV).load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=seed)
    ref = {k: np.array(v, np.float64) for k, v in p0.items()}
    opt = T.AMSGrad(T.trainable_names(md), ref, lr=md["learning_rate"])
    rng = np.random.default_rng(7)
    present = np.arange(R // 2)
    batch = _batch(md, B, 37, seed=100)
    batch["rel"] = rng.choice(present, B)
    assert set(batch["rel"]) == set(present)
    ob = dict(e1=batch["e1"], rel=batch["rel"], lookup=batch["lookup_values"], labels=batch["e2_multi"])
    _, grads_o, gn_o = T.train_step(ref, md, ob, opt, seed=seed, step=0, momentum=md["batch_norm_momentum"])
    m.train_step(batch)
    first = {leaf: m.train_grad(leaf)[0].clone() for leaf in T.trainable_names(md)}
    torch.cuda.synchronize()
    q = cdata.synthetic_queries(md, 300, seed=11)
    q["rel"] = rng.integers(R // 2, R, 300)                      # the complement
    h = m.encode(q["e1"], q["rel"])
    m.rank(h, q["e2"], q["filt_indptr"], q["filt_idx"])
    m.encode(rng.integers(0, E, 77), rng.integers(0, R, 77))
    m.reserve(40000, 0)
    torch.cuda.synchronize()
    for leaf, g0 in first.items():
        g1, _ = m.train_grad(leaf)
        assert _same(g1, g0), leaf
    g, _ = m.train_grad("fc_weights")
    g = g.cpu().numpy().reshape(grads_o["fc_weights"].shape)
    assert np.abs(g[R // 2:]).max() == 0.0
    assert _rel_err(g, grads_o["fc_weights"], 1e-3 * gn_o) < 2e-4
    m.close()
