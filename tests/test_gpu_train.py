"""GPU tests of the training step through the C ABI, against oracle/coper_train_oracle.py
(float64 torch-autograd restatement of models.py:176-200,354-457 + utils/amsgrad.py).  Tolerances are fp32
rounding of a ~5k-term reduction chain; the oracle gets the same dropout masks (same counter hash)."""
import numpy as np
import pytest
import torch

from coper_amd import data as cdata

pytestmark = pytest.mark.gpu

_CASES = {
    "cpg_linear": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                       context_rel_conv=None, context_rel_out=[]),
    "plain": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=40, emb_h=10, emb_w=4, conv_num_channels=8,
                  context_rel_conv=None, context_rel_out=None),
    "cpg_mlp_bn": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                       context_rel_conv=None, context_rel_out=[12], context_rel_use_batch_norm=True, context_rel_dropout=0.2),
    "cpg_mlp2": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                     context_rel_conv=None, context_rel_out=[9, 7], context_rel_use_batch_norm=False, context_rel_dropout=0.1),
    "lookup": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=1, emb_h=10, emb_w=4, conv_num_channels=8,
                   context_rel_conv=None, context_rel_out=[], do_parameter_lookup=True),
    "cpg_conv_fc": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                        context_rel_conv=[], context_rel_out=[]),
    "cpg_conv_mlp": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                         context_rel_conv=[5], context_rel_out=[7], context_rel_use_batch_norm=True, context_rel_dropout=0.2),
    "lookup_conv": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=1, emb_h=10, emb_w=4, conv_num_channels=8,
                        context_rel_conv=[], context_rel_out=[], do_parameter_lookup=True),
    # looked-up conv filters with a STATIC dense layer (models.py:217-228 with context_rel_out None)
    "lookup_conv_static_fc": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=1, emb_h=10, emb_w=4, conv_num_channels=8,
                                  context_rel_conv=[], context_rel_out=None, do_parameter_lookup=True),
    # a looked-up dense layer whose input is NARROWER than four outputs (F = 5 * 9 * 3 = 135 < 4 * 77): its forward keeps four partial sums
    # of [B, d] in the workspace that also holds dx [B, F] -- until round 6 sized for dx alone (found by the 96-shape fuzz run)
    "lookup_narrow_F": dict(num_ent=130, num_rel=6, ent_emb_size=77, rel_emb_size=1, emb_h=7, emb_w=11, conv_num_channels=3,
                            context_rel_conv=[], context_rel_out=[], do_parameter_lookup=True),
    "cpg_linear_concat": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                              context_rel_conv=None, context_rel_out=[], concat_rel=True),
    "plain_concat": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=40, emb_h=10, emb_w=4, conv_num_channels=8,
                         context_rel_conv=None, context_rel_out=None, concat_rel=True),
    "cpg_conv_static_fc": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                               context_rel_conv=[6], context_rel_out=None, concat_rel=True, context_rel_use_batch_norm=True,
                               context_rel_dropout=0.1),
    # full-width layers (F = 10368 / 4608, d = 200): the GEMMs span several 128 x 128 tiles and the few-tile products
    # (z0 = x W, dh = S E) take the split-K route
    "plain_wide": dict(num_ent=700, num_rel=6, ent_emb_size=200, rel_emb_size=200, emb_h=10, emb_w=20, conv_num_channels=32,
                       context_rel_conv=None, context_rel_out=None),
    "cpg_wide": dict(num_ent=700, num_rel=6, ent_emb_size=200, rel_emb_size=8, emb_h=10, emb_w=20, conv_num_channels=32,
                     context_rel_conv=None, context_rel_out=[]),
    "cpg_linear_c32": dict(num_ent=157, num_rel=4, ent_emb_size=80, rel_emb_size=4, emb_h=10, emb_w=8, conv_num_channels=32,
                           context_rel_conv=None, context_rel_out=[]),
    # entity tables whose row of the dense scorer backward does not fit 64 KB of LDS, and not one LDS stretch either (k_tr_build_S:
    # 20,011 entities = 78 KB in one stretch; 41,003 = two stretches of <= 32,768 columns -- WN18RR has 40,943)
    "cpg_linear_e20k": dict(num_ent=20011, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                            context_rel_conv=None, context_rel_out=[]),
    "plain_e41k": dict(num_ent=41003, num_rel=6, ent_emb_size=40, rel_emb_size=40, emb_h=10, emb_w=4, conv_num_channels=8,
                       context_rel_conv=None, context_rel_out=None),
}


def _fuzz_cases(n):
    """Seeded random shapes for the training step: embedding sizes that are not multiples of 4 or 8, other filter sizes,
    channel counts that do not divide the workgroup, every model variant in turn; one case above d = 256."""
    out = {}
    for seed in range(n):
        rng = np.random.default_rng(500 + seed)
        emb_h, emb_w = int(rng.integers(3, 11)), int(rng.integers(3, 13))
        d = emb_h * emb_w
        fh, fw = [(3, 3), (2, 2), (1, 3), (3, 2), (3, 3)][int(rng.integers(0, 5))]
        md = dict(num_ent=int(rng.choice([37, 130, 301])), num_rel=int(rng.choice([2, 6, 10])), ent_emb_size=d,
                  rel_emb_size=int(rng.choice([3, 8])), emb_h=emb_h, emb_w=emb_w, conv_filter_height=fh, conv_filter_width=fw,
                  conv_num_channels=int(rng.choice([3, 8, 12, 32])))
        v = seed % 6
        if v == 0:
            md.update(context_rel_conv=None, context_rel_out=[])
        elif v == 1:
            md.update(context_rel_conv=[], context_rel_out=[])
        elif v == 2:
            md.update(context_rel_conv=[5], context_rel_out=[7], context_rel_use_batch_norm=bool(seed & 8), context_rel_dropout=0.1)
        elif v == 3:
            md.update(context_rel_conv=[], context_rel_out=[], do_parameter_lookup=True, rel_emb_size=1)
        elif v == 4:
            md.update(context_rel_conv=None, context_rel_out=None, rel_emb_size=d)
        else:
            md.update(context_rel_conv=None, context_rel_out=[], concat_rel=True)
        out["fuzz_%02d" % seed] = md
    out["fuzz_d288"] = dict(num_ent=130, num_rel=6, ent_emb_size=288, rel_emb_size=8, emb_h=12, emb_w=24, conv_filter_height=2,
                            conv_filter_width=3, conv_num_channels=5, context_rel_conv=None, context_rel_out=[])
    return out


import os as _os
_CASES.update(_fuzz_cases(int(_os.environ.get("COPER_TRAIN_FUZZ", "12"))))      # (COPER_TRAIN_FUZZ=96: the same tests as a soak of random shapes)


def _batch(md, B, L, seed):
    rng = np.random.default_rng(seed)
    E, R = md["num_ent"], md["num_rel"]
    lookup = rng.integers(0, E, (B, L)).astype(np.int32)
    lookup[:, 0] = rng.integers(0, E, B)                      # the positive first, as the sampler does
    labels = np.zeros((B, L), np.float32)
    labels[:, 0] = 1.0
    labels[rng.random((B, L)) < 0.05] = 1.0
    return dict(e1=rng.integers(0, E, B), rel=rng.integers(0, R, B), lookup_values=lookup, e2_multi=labels)


def _rel_err(a, b, floor):
    # `floor`: gradients that are exactly zero in exact arithmetic (conv1_bias under batch-statistics BN is
    # shift-invariant) come out as rounding noise on both sides
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor)


@pytest.mark.parametrize("train_stats,one_vs_all", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("name", sorted(_CASES))
def test_train_step_matches_oracle(name, train_stats, one_vs_all):
    """The table law of SURVEY 8(d) (sigma = 0.1).  Rounds 2 - 4 kept sigma = 0.3 here behind an environment variable: on the 0.1
    table one fuzz case had an activation 6e-6 from a ReLU kink, inside the 1.5e-5 error of the bf16-split GEMMs, and passed or
    failed with the run.  Round 5 moved those GEMMs to the scaled fp16 split (5e-7): the variable is gone."""
    _train_step_case(name, train_stats, one_vs_all, "n0.1")


@pytest.mark.parametrize("name", sorted(k for k in _CASES if not k.startswith("fuzz_")) + ["fuzz_00", "fuzz_d288"])
def test_train_step_matches_oracle_from_the_reference_init(name):
    """... and from the state the reference itself starts training in (models.py:205-214, 284-293: xavier-uniform tables and
    projections, zero biases, BN at its defaults -- `data.reference_init_params`), where the embeddings are +-0.1 and smaller."""
    _train_step_case(name, True, False, "reference")


@pytest.mark.parametrize("name,L", [("cpg_linear", 700), ("plain", 301), ("cpg_wide", 1000), ("fuzz_d288", 259), ("cpg_linear", 9000), ("lookup", 8193)])
def test_train_step_matches_oracle_with_long_lookups(name, L):
    """Lookups longer than a workgroup (k_tr_score_loss_dh takes the rows of a query in batches of <= 256, a thread per row of the
    batch when it scores them: at d = 40 a batch is 252 rows, at d = 200 60) -- the sampled cases above have L = 37.  Beyond 8,192 entries
    the row ids no longer fit the kernel's LDS plan: the two-kernel path of rounds 1 - 5 takes those."""
    _train_step_case(name, True, False, "n0.1", B=24, L=L, steps=2)


def _shape_cases():
    n = int(_os.environ.get("COPER_TRAIN_SHAPE_FUZZ", "10"))      # (COPER_TRAIN_SHAPE_FUZZ=200: a soak of batch shapes)
    rng = np.random.default_rng(77)
    names = ["cpg_linear", "plain", "cpg_mlp_bn", "lookup", "cpg_conv_fc", "lookup_narrow_F", "cpg_linear_c32", "fuzz_03", "fuzz_06", "fuzz_d288"]
    out = []
    for i in range(n):
        B = int(rng.choice([2, 3, 5, 17, 31, 64, 65, 100, 129]))
        L = int(rng.choice([1, 2, 5, 36, 63, 64, 65, 130, 251, 252, 253, 256, 257, 505, 1001]))
        # (batch statistics over 2 - 5 samples are ill-conditioned -- FCBN of two samples is +-1 whatever they were: rounding differences of
        #  the step come back amplified past the tolerances that hold from 8 samples on; those batches take the moving statistics)
        out.append((names[i % len(names)], B, L, bool(rng.random() < 0.7) and B >= 8))
    return out


@pytest.mark.parametrize("name,B,L,train_stats", _shape_cases())
def test_train_step_matches_oracle_over_batch_shapes(name, B, L, train_stats):
    """Batch shapes around every grain of the step's kernels: 2 ... 129 queries, 1 ... 1,001 lookup entries (a batch of the fused scorer is
    60 - 252 rows, a workgroup 256 threads, a GEMM tile 128 rows)."""
    md = _CASES[name]
    if L > md["num_ent"]:
        L = md["num_ent"]
    _train_step_case(name, train_stats, False, "n0.1", B=B, L=L, steps=2)


def _train_step_case(name, train_stats, one_vs_all, init, B=48, L=37, steps=3, edit=None, case=None, form=None, clip_norm=5.0,
                     grads_out=None, batch_seed=100):
    """`edit(m, ref)`: a change of the variables made to both sides before the last step (tests/test_gpu_between_calls.py); the
    oracle then restarts from the device's variables before every step, each held to the step-0 bounds.
    `case`: the model's dimensions (else _CASES[name]; a `case` restarts the oracle like `edit`); `form`: the oracle's
    (coper_train_oracle.forward_train); `clip_norm`: both sides'; `grads_out`: a dict that receives the device's step-0 gradients;
    step i trains on _batch(seed=batch_seed + i).  Returns the oracle's global gradient norm of every step."""
    from coper_amd.models import ConvE
    from oracle import coper_train_oracle as T
    md = dict(cdata._COMMON)
    md.update(_CASES[name] if case is None else case)
    md.update(batch_norm_train_stats=train_stats, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1) if init == "n0.1" else cdata.reference_init_params(md, 21)
    seed = 5
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=seed, clip_norm=clip_norm)
    ref = {k: np.array(v, np.float64) for k, v in p0.items()}
    opt = T.AMSGrad(T.trainable_names(md), ref, lr=md["learning_rate"], clip=clip_norm)
    # the wide and the random-shape cases restart the oracle from the device's variables before every step, so that each step is held to the
    # step-0 bounds (the other cases let the two trajectories run free and bound the Adam-amplified drift instead)
    sync = name.endswith("_wide") or name.startswith("fuzz_") or edit is not None or case is not None
    norms = []
    for step in range(steps):
        batch = _batch(md, B, L, seed=batch_seed + step)
        if edit is not None and step == steps - 1:
            edit(m, ref)
        if sync and step > 0:
            for k in ref:
                ref[k] = m._tensors[k].cpu().numpy().reshape(np.shape(ref[k])).astype(np.float64)
        tight = step == 0 or sync
        if one_vs_all:       # use_negative_sampling = False: dense labels over all entities, no lookup (data.py:313-334)
            dense = np.zeros((B, md["num_ent"]), np.float32)
            np.put_along_axis(dense, batch["lookup_values"].astype(np.int64), batch["e2_multi"], axis=1)
            batch = dict(e1=batch["e1"], rel=batch["rel"], e2_multi=dense, lookup_values=np.zeros((B, 0), np.int32))
        ob = dict(e1=batch["e1"], rel=batch["rel"], lookup=None if one_vs_all else batch["lookup_values"], labels=batch["e2_multi"])
        loss_o, grads_o, gn_o = T.train_step(ref, md, ob, opt, seed=seed, step=step, momentum=md["batch_norm_momentum"], form=form)
        norms.append(gn_o)
        loss = float(m.train_step(batch).cpu()[0])
        assert abs(loss - loss_o) < (2e-5 if tight else 2e-4) * max(1.0, abs(loss_o)), (step, loss, loss_o)
        dg = {}
        for leaf in T.trainable_names(md):
            g, gn = m.train_grad(leaf)
            g = g.cpu().numpy().reshape(grads_o[leaf].shape)
            if grads_out is not None and step == 0:
                grads_out[leaf] = g
            err = _rel_err(g, grads_o[leaf], 1e-3 * gn_o)
            # step 0 starts from identical variables; later steps inherit the (bounded, Adam-amplified) differences of the
            # variables themselves, which the gradients see
            assert err < (2e-4 if tight else 3e-3), (step, leaf, err)
            dg[leaf] = np.abs(g - grads_o[leaf]).max()
        assert abs(gn - gn_o) < 1e-4 * gn_o
        # the variables themselves (updated in place), including the BN moving statistics
        for leaf, want in ref.items():
            if train_stats and leaf == "conv1_bias":
                # exact gradient 0 (batch-statistics BN is shift-invariant): Adam-type updates m/(sqrt(v_hat)+eps)
                # turn the fp32 rounding noise of either side into an O(lr) step -- nothing to compare
                continue
            got = m._tensors[leaf].cpu().numpy().reshape(np.shape(want))
            # g -> lr_t * m / (sqrt(v_hat) + eps) has slope <= lr_t * (1 - beta1) / eps where |g| ~ eps = 1e-8: an
            # absolute gradient error dg (fp32 rounding) may move such an entry by that much
            lr_t = md["learning_rate"] * 0.32
            # moving statistics after step 0 are batch statistics of activations computed from variables that already
            # differ by the bound above (summed over up to F = 10368 inputs in the wide cases)
            rel = 5e-5 if (not tight and leaf not in dg) else 1e-5
            tol = 2e-5 + rel * np.abs(want).max() + 2.0 * lr_t * 0.1 * dg.get(leaf, 0.0) / 1e-8
            if train_stats and leaf == "Conv1BN/moving_mean" and "conv1_bias" in ref:
                # mean(conv) carries conv1_bias, whose noise-driven steps are excluded above
                bias = m._tensors["conv1_bias"].cpu().numpy().reshape(-1)
                tol += np.abs(bias - np.reshape(ref["conv1_bias"], -1)).max()
            assert np.abs(got - want).max() < tol, (step, leaf, np.abs(got - want).max(), tol)
    # inference after training: caches are rebuilt from the updated variables
    q = cdata.synthetic_queries(md, 40, seed=3)
    h = m.encode(q["e1"], q["rel"]).cpu().numpy()
    from oracle import coper_oracle as O
    hr = O.forward({k: np.asarray(v, np.float32) for k, v in ref.items()}, md, q["e1"], q["rel"], np.float64)["h"]
    # (the variables carry the Adam-amplified rounding differences bounded above: a sanity check of the rebuild)
    assert np.abs(h - hr).max() < 1e-3
    m.close()
    return norms


def test_train_rejects_unsupported_variants_and_order():
    from coper_amd.models import ConvE
    from coper_amd._lib import CoperError
    md = dict(cdata._COMMON)
    md.update(_CASES["cpg_linear"])
    p = cdata.synthetic_params(md, seed=1, ent_std=0.3)
    m = ConvE(md, device="cuda:0")
    m.load_parameters(p)
    with pytest.raises(CoperError):
        m.train_step(_batch(md, 4, 5, 0))   # no train_init
    m.close()
    sh = ConvE(md, device="cuda:0", shard=(0, 100))
    sh.load_parameters(p)
    with pytest.raises(CoperError, match="whole entity table"):
        sh.train_init()                     # training needs the whole table on the handle
    sh.close()
    md5 = dict(md, conv_num_channels=300)
    m5 = ConvE(md5, device="cuda:0")
    m5.load_parameters(cdata.synthetic_params(md5, seed=1, ent_std=0.3))
    with pytest.raises(CoperError, match="256 conv channels"):
        m5.train_init()                     # (any filter size, channel count up to 256, d up to coper_create's 320)
    m5.close()


@pytest.mark.parametrize("variant", ["cpg_linear", "plain", "lookup", "cpg_mlp_bn", "cpg_linear@reference_init", "plain@reference_init"])
def test_training_loop_learns_a_small_graph(variant):
    """End to end: TrainDataset (the reference's one-positive-per-row sampler) -> train_step -> prepare ->
    ranking_and_hits.  The loss falls and the filtered MRR on the training triples ends far above chance -- also from the state
    the reference starts in (`@reference_init`: xavier tables, zero biases, BN defaults; models.py:205-214, 284-293)."""
    variant, _, init = variant.partition("@")
    from coper_amd.data import EvalDataset, TrainDataset
    from coper_amd.metrics import ranking_and_hits
    from coper_amd.models import ConvE
    E, R = 120, 4
    md = dict(cdata._COMMON)
    md.update(_CASES[variant])
    md.update(num_ent=E, num_rel=R, batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.1, output_dropout=0.1,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    rng = np.random.default_rng(0)
    mult, off = [1, 7, 11, 13], [3, 17, 29, 41]
    e1 = np.repeat(np.arange(E), R)
    rel = np.tile(np.arange(R), E)
    e2 = (e1 * np.array(mult)[rel] + np.array(off)[rel]) % E
    samples = dict(e1=e1, rel=rel, tail_indptr=np.arange(len(e1) + 1), tail_idx=e2.astype(np.int64))
    p = cdata.reference_init_params(md, 4) if init else cdata.synthetic_params(md, seed=4, ent_std=0.3)
    m = ConvE(md, device="cuda:0").load_parameters(p)

    def mrr():
        q = dict(e1=e1, rel=rel, e2=e2, filt_indptr=np.arange(len(e1) + 1), filt_idx=e2.astype(np.int64))
        return ranking_and_hits(m, None, EvalDataset(q, 256, E), "train")[1]

    before = mrr()
    m.train_init(seed=3)
    it = iter(TrainDataset(samples, E, batch_size=96, num_labels=40, seed=5))
    losses = []
    for step in range(600):
        loss = m.train_step(next(it))
        if step % 50 == 0 or step == 599:
            losses.append(float(loss.cpu()[0]))
    after = mrr()
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], losses
    assert before < 0.15 and after > (0.3 if init else 0.5) and after > 4 * before, (before, after, losses)
    m.close()


def test_checkpoint_resume_continues_the_same_trajectory(tmp_path):
    """Variables + AMSGrad slots + beta powers through the TF-checkpoint writer / reader (run_cpg.py:189,206,252):
    a model restored from the checkpoint takes the same next steps as the one that kept running."""
    from coper_amd import weights
    from coper_amd.models import ConvE
    md = dict(cdata._COMMON)
    md.update(_CASES["cpg_mlp_bn"])
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.2, output_dropout=0.1,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    p0 = cdata.synthetic_params(md, seed=3, ent_std=0.3)
    a = ConvE(md, device="cuda:0").load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    a.train_init(seed=7)
    for step in range(3):
        a.train_step(_batch(md, 32, 20, seed=step))
    slots, powers = a.optimizer_state()
    assert powers["step"] == 3 and abs(powers["beta1_power"] - 0.9 ** 4) < 1e-6
    prefix = str(tmp_path / "model_weights.ckpt")
    weights.save_tf_checkpoint(prefix, {k: v.cpu().numpy() for k, v in a._tensors.items()}, slots, powers)
    params, slots2, powers2 = weights.load_tf_checkpoint(prefix, with_optimizer=True)
    assert sorted(slots2) == sorted(slots) and all(np.array_equal(slots2[k][2], slots[k][2]) for k in slots)
    b = ConvE(md, device="cuda:0").load_parameters({k: torch.as_tensor(v) for k, v in params.items()})
    b.train_init(seed=7)
    b.load_optimizer_state(slots2, dict(powers2, step=powers["step"]))
    for step in range(3, 5):
        la = float(a.train_step(_batch(md, 32, 20, seed=step)).cpu()[0])
        lb = float(b.train_step(_batch(md, 32, 20, seed=step)).cpu()[0])
        assert abs(la - lb) < 1e-5 * max(1.0, abs(la))
    for k in a._tensors:
        if k == "conv1_bias":      # exact gradient 0 under batch-statistics BN: Adam turns rounding noise into steps
            continue
        x, y = a._tensors[k].cpu().numpy(), b._tensors[k].cpu().numpy()
        assert np.abs(x - y).max() < 1e-5 + 1e-4 * np.abs(x).max(), k
    a.close()
    b.close()


def test_example_train_eval_checkpoint_loop(tmp_path):
    """examples/train_eval_loop.py: loader -> training steps -> filtered ranking -> TF-format checkpoint -> restore
    (the loop of run_cpg.py:108-260), on the nell-995 split under tests/golden; learns well above chance."""
    import importlib.util
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    spec = importlib.util.spec_from_file_location("train_eval_loop", os.path.join(root, "examples", "train_eval_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mrr = mod.main(["--steps", "150", "--eval-every", "150", "--workdir", str(tmp_path)])
    assert mrr > 0.1          # chance on 765 entities is ~0.01


@pytest.mark.parametrize("tag", ["plain", "cpg", "cpg_mlp"])
def test_train_step_gradients_match_reference_sister_models_autograd(tag):
    """coper_train_step's loss and gradients against torch autograd through the REFERENCE's own PyTorch forward
    (fact_network.py ConvE / CPG_ConvE) and loss (emb.py:50-58): tests/golden/minerva_grads.npz, eval-mode BN, no
    dropout, dense 1-vs-all labels."""
    import os
    from coper_amd.models import ConvE
    from tests.minerva_map import load_grad_case, reference_grads_in_our_layout
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minerva_grads.npz"))
    md, p, sd, batch = load_grad_case(g, tag)
    m = ConvE(md, device="cuda:0").load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p.items()})
    m.train_init(seed=0)
    loss = float(m.train_step(dict(e1=batch["e1"], rel=batch["rel"], e2_multi=batch["labels"],
                                   lookup_values=np.zeros((len(batch["e1"]), 0), np.int32))).cpu()[0])
    assert abs(loss - float(g[tag + ":loss"])) < 1e-5 * abs(loss)
    ours = {leaf: m.train_grad(leaf)[0].cpu().numpy() for leaf in m.trainable_leaves()}
    for leaf, (want, got) in reference_grads_in_our_layout(g, tag, sd, ours).items():
        want, got = np.asarray(want, np.float64), np.asarray(got, np.float64).reshape(np.shape(want))
        assert np.abs(got - want).max() < 2e-4 * max(np.abs(want).max(), 1e-6) + 1e-8, leaf
    m.close()


def test_session_run_serves_the_training_fetches():
    """`loss, _ = session.run((model.loss, model.train_op), {model.is_train: True, model.input_iterator_handle: h})`
    (run_cpg.py:211-219) is one coper_train_step on the iterator's next batch; variables fetched directly come back as
    host arrays (run_cpg.py:244-248)."""
    from coper_amd.models import ConvE, OutOfRangeError
    md = dict(cdata._COMMON)
    md.update(_CASES["cpg_linear"])
    md.update(learning_rate=0.003, use_negative_sampling=True)
    p0 = cdata.synthetic_params(md, seed=3, ent_std=0.3)
    batches = [_batch(md, 32, 20, seed=50 + i) for i in range(3)]
    a = ConvE(md, device="cuda:0").load_parameters({k: torch.as_tensor(np.array(v)) for k, v in p0.items()})
    b = ConvE(md, device="cuda:0").load_parameters({k: torch.as_tensor(np.array(v)) for k, v in p0.items()})
    a.train_init(seed=9)
    b.train_init(seed=9)
    sess = a.session()
    feed = {a.is_train: True, a.input_iterator_handle: batches}
    for i in range(3):
        loss, none = sess.run((a.loss, a.train_op), feed)
        assert none is None and isinstance(loss, float)
        other = float(b.train_op(batches[i]).cpu()[0])                   # the callable form, same arithmetic
        assert abs(loss - other) <= 2e-6 * max(1.0, abs(other))          # (atomic float sums: the order is not fixed)
    with pytest.raises(OutOfRangeError):
        sess.run((a.loss, a.train_op), feed)
    rel_emb, ent_emb = sess.run([a.variables["rel_emb"], a.variables["ent_emb"]])
    # two models stepping on the same batches agree up to the order of the atomic float sums
    assert np.allclose(ent_emb, b.variables["ent_emb"].cpu().numpy(), rtol=0, atol=1e-5) and rel_emb.shape == (md["num_rel"], md["rel_emb_size"])
    assert np.array_equal(ent_emb, a.variables["ent_emb"].cpu().numpy())   # the fetch IS the variable
    assert not np.array_equal(ent_emb, p0["ent_emb"])                     # the variables moved
    with pytest.raises(ValueError):
        sess.run((a.loss, a.train_op), {a.input_iterator_handle: batches})   # train_op without is_train
    # evaluation fetches on the updated variables still work through the same session
    q = cdata.synthetic_queries(md, 16, seed=1)
    pred = sess.run(a.predictions_all, {a.input_iterator_handle: [dict(q, lookup_values=np.zeros((16, 0), np.int32))]})
    assert pred.shape == (16, md["num_ent"])
    a.close()
    b.close()


def test_handles_release_their_device_memory():
    """coper_destroy gives back everything a handle allocated -- caches, workspaces, the training state (plane sets,
    split-K partial sums, optimizer slots): after create / prepare / rank / top-k / train / destroy cycles the library's
    allocation ledger (coper_live_device_bytes) is back where it was, to the byte."""
    from coper_amd.models import ConvE
    md = dict(cdata._COMMON)
    md.update(_CASES["cpg_wide"])
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    p0 = {k: torch.as_tensor(np.array(v, np.float32)) for k, v in cdata.synthetic_params(md, seed=3, ent_std=0.3).items()}
    q = cdata.synthetic_queries(md, 300, seed=1)
    batch = _batch(md, 48, 37, seed=7)

    def cycle(mode):
        m = ConvE(md, device="cuda:0", score_mode=mode)
        m.load_parameters({k: v.clone() for k, v in p0.items()})
        m.prepare()
        m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
        h = m.encode(q["e1"], q["rel"])
        m.rank_counts(h, m.target_scores(h, q["e2"]), q["e2"], q["filt_indptr"], q["filt_idx"], k=10)   # top-k workspaces
        m.train_init(seed=1)
        m.train_step(batch)
        m.train_step(dict(e1=batch["e1"], rel=batch["rel"], e2_multi=np.zeros((48, md["num_ent"]), np.float32),
                          lookup_values=np.zeros((48, 0), np.int32)))
        m.close()

    from coper_amd import _lib
    import gc
    lib = _lib.load()
    gc.collect()                              # handles earlier tests dropped without close()
    base = lib.coper_live_device_bytes()      # other live handles of this process, if any
    held = []
    for i in range(6):
        m = ConvE(md, device="cuda:0", score_mode="bf16x3" if i % 2 == 0 else "f32")
        assert lib.coper_live_device_bytes() >= base
        m.close()
        cycle("bf16x3" if i % 2 == 0 else "f32")
        held.append(lib.coper_live_device_bytes())
    # the library's own ledger (every allocation it makes is entered there): exact, unlike hipMemGetInfo, which also moves
    # with the runtime's scratch and pool decisions
    assert held == [base] * len(held), (base, held)
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: v.clone() for k, v in p0.items()})
    m.prepare()
    assert lib.coper_live_device_bytes() - base > (8 << 20)     # a prepared handle of this size holds 24 MB
    m.close()
    assert lib.coper_live_device_bytes() == base


def test_train_batch_shape_changes_between_steps():
    """One handle, consecutive steps whose batch changes shape -- B 16 / 70 / 48 / 5, sampled lists of 9 / 60 / 37 entities and
    1-vs-all rows in between (the training workspaces, plane sets and split-K pools regrow; label modes alternate): loss and
    every gradient of every step against the oracle restarted from the device's variables."""
    from coper_amd.models import ConvE
    from oracle import coper_train_oracle as T
    md = dict(cdata._COMMON)
    md.update(_CASES["cpg_wide"])
    md.update(num_ent=300, batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    p0 = cdata.synthetic_params(md, seed=4, ent_std=0.3)
    seed = 9
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=seed)
    ref = {k: np.array(v, np.float64) for k, v in p0.items()}
    opt = T.AMSGrad(T.trainable_names(md), ref, lr=md["learning_rate"])
    shapes = [(16, 9, False), (70, 60, False), (48, 0, True), (5, 37, False), (70, 0, True), (16, 60, False)]
    for step, (B, L, one_vs_all) in enumerate(shapes):
        for k in ref:
            ref[k] = m._tensors[k].cpu().numpy().reshape(np.shape(ref[k])).astype(np.float64)
        batch = _batch(md, B, max(L, 3), seed=300 + step)
        if one_vs_all:
            dense = np.zeros((B, md["num_ent"]), np.float32)
            np.put_along_axis(dense, batch["lookup_values"].astype(np.int64), batch["e2_multi"], axis=1)
            batch = dict(e1=batch["e1"], rel=batch["rel"], e2_multi=dense, lookup_values=np.zeros((B, 0), np.int32))
        ob = dict(e1=batch["e1"], rel=batch["rel"], lookup=None if one_vs_all else batch["lookup_values"], labels=batch["e2_multi"])
        loss_o, grads_o, gn_o = T.train_step(ref, md, ob, opt, seed=seed, step=step, momentum=md["batch_norm_momentum"])
        loss = float(m.train_step(batch).cpu()[0])
        assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (step, B, L, loss, loss_o)
        for leaf in T.trainable_names(md):
            g, gn = m.train_grad(leaf)
            err = _rel_err(g.cpu().numpy().reshape(grads_o[leaf].shape), grads_o[leaf], 1e-3 * gn_o)
            assert err < 2e-4, (step, B, L, leaf, err)
        assert abs(gn - gn_o) < 1e-4 * gn_o
    m.close()


def test_device_sampler_feeds_the_training_loop():
    """DeviceTrainDataset on the HIP device: batches of device tensors in the reference's batch contract, construction
    rules as on the host, and a training loop fed by it learns the small graph like the host-fed one."""
    from coper_amd.data import DeviceTrainDataset, EvalDataset
    from coper_amd.metrics import ranking_and_hits
    from coper_amd.models import ConvE
    E, R = 120, 4
    md = dict(cdata._COMMON)
    md.update(_CASES["cpg_linear"])
    md.update(num_ent=E, num_rel=R, batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.1, output_dropout=0.1,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    mult, off = [1, 7, 11, 13], [3, 17, 29, 41]
    e1 = np.repeat(np.arange(E), R)
    rel = np.tile(np.arange(R), E)
    e2 = (e1 * np.array(mult)[rel] + np.array(off)[rel]) % E
    samples = dict(e1=e1, rel=rel, tail_indptr=np.arange(len(e1) + 1), tail_idx=e2.astype(np.int64))
    ds = DeviceTrainDataset(samples, E, batch_size=96, num_labels=40, seed=5, device="cuda:0")
    it = iter(ds)
    b = next(it)
    assert all(v.is_cuda for v in b.values())
    assert b["lookup_values"].shape == (96, 40) and b["lookup_values"].dtype == torch.int32 and b["e2_multi"].dtype == torch.float32
    lk, lab = b["lookup_values"].cpu().numpy(), b["e2_multi"].cpu().numpy()
    assert np.array_equal(lk[:, 0], b["e2"].cpu().numpy()) and (lab[:, 0] == 1).all()
    want = (lk == ((b["e1"].cpu().numpy() * np.array(mult)[b["rel"].cpu().numpy()] + np.array(off)[b["rel"].cpu().numpy()]) % E)[:, None])
    assert np.array_equal(lab, want.astype(np.float32))              # one known tail per (e1, rel) in this graph
    assert all(len(set(row[1:].tolist())) == 39 for row in lk)
    m = ConvE(md, device="cuda:0").load_parameters(cdata.synthetic_params(md, seed=4, ent_std=0.3))

    def mrr():
        q = dict(e1=e1, rel=rel, e2=e2, filt_indptr=np.arange(len(e1) + 1), filt_idx=e2.astype(np.int64))
        return ranking_and_hits(m, None, EvalDataset(q, 256, E), "train")[1]

    before = mrr()
    m.train_init(seed=3)
    losses = []
    for step in range(600):
        loss = m.train_step(next(it))
        if step % 50 == 0 or step == 599:
            losses.append(float(loss.cpu()[0]))
    after = mrr()
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], losses
    assert before < 0.15 and after > 0.5 and after > 4 * before, (before, after, losses)
    m.close()


def test_device_sampler_proportional_mode_on_the_gpu():
    """The proportional sampler (the shipped configs' default) on the HIP device: construction rules, and steps fed by it run."""
    from coper_amd.data import DeviceTrainDataset
    from coper_amd.models import ConvE
    rng = np.random.default_rng(6)
    E, N, L = 211, 60, 37
    indptr, idx = [0], []
    for i in range(N):
        k = int(rng.integers(1, 12))
        idx.extend(sorted(rng.choice(E, size=k, replace=False)))
        indptr.append(len(idx))
    s = dict(e1=np.arange(N), rel=rng.integers(0, 6, N), tail_indptr=np.array(indptr), tail_idx=np.array(idx))
    prop = 5.0
    need = int(1.0 / (1.0 + prop) * L)
    it = iter(DeviceTrainDataset(s, E, batch_size=48, num_labels=L, seed=2, device="cuda:0", one_positive_label_per_sample=False,
                                 prop_negatives=prop))
    md = dict(cdata._COMMON)
    md.update(_CASES["cpg_linear"])
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.1, output_dropout=0.1, label_smoothing_epsilon=0.1,
              learning_rate=0.003)
    m = ConvE(md, device="cuda:0").load_parameters(cdata.synthetic_params(md, seed=4, ent_std=0.3))
    m.train_init(seed=1)
    for _ in range(5):
        b = next(it)
        assert all(v.is_cuda for v in b.values())
        h = {k: v.cpu().numpy() for k, v in b.items()}
        for r in range(48):
            t = idx[indptr[int(h["e1"][r])]:indptr[int(h["e1"][r]) + 1]]
            lk, lab = h["lookup_values"][r], h["e2_multi"][r]
            lead = len(t) if len(t) <= need else max(L - min(E, L - need), 0)
            assert set(lk[:lead].tolist()) <= set(t) and len(set(lk[:lead].tolist())) == lead and len(set(lk[lead:].tolist())) == L - lead
            assert np.array_equal(lab, np.array([float(v in t) for v in lk], np.float32)) and int(h["e2"][r]) == int(lk[0])
        assert np.isfinite(float(m.train_step(b).cpu()[0]))
    m.close()


@pytest.mark.parametrize("one_vs_all", [False, True])
@pytest.mark.parametrize("name", ["cpg_linear", "plain", "cpg_mlp_bn", "lookup"])
def test_train_forward_is_the_step_without_the_update(name, one_vs_all):
    """coper_train_forward (round 5): `session.run((model.loss, model.predictions_lookup), {is_train: True})` without train_op
    (models.py:183-192).  Its loss is bit-for-bit the loss the NEXT train_step reports on the same batch (same dropout masks,
    same batch statistics); its logits reproduce that loss through the label-smoothed BCE of models.py:448-453; and nothing is
    written: every variable, BN moving statistic and optimizer slot keeps its bits."""
    from coper_amd.models import ConvE
    md = dict(cdata._COMMON)
    md.update(_CASES[name])
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    p0 = cdata.synthetic_params(md, seed=8, ent_std=0.1)
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=11)
    B, L = 40, 29
    m.train_step(_batch(md, B, L, seed=1))                      # (slots and moving statistics away from their initial values)
    batch = _batch(md, B, L, seed=2)
    if one_vs_all:
        dense = np.zeros((B, md["num_ent"]), np.float32)
        np.put_along_axis(dense, batch["lookup_values"].astype(np.int64), batch["e2_multi"], axis=1)
        batch = dict(e1=batch["e1"], rel=batch["rel"], e2_multi=dense, lookup_values=np.zeros((B, 0), np.int32))
    before = {k: v.clone() for k, v in m._tensors.items()}
    slots0, pow0 = m.optimizer_state()
    sess = m.session()
    fetched = sess.run((m.loss, m.predictions_lookup, m.predicted_e2_emb), {m.is_train: True, m.input_iterator_handle: [batch]})
    loss_f, pred, hv = fetched
    for k, v in m._tensors.items():
        assert torch.equal(v, before[k]), k
    slots1, pow1 = m.optimizer_state()
    assert pow0 == pow1 and all(np.array_equal(a, b) for k in slots0 for a, b in zip(slots0[k], slots1[k]))
    Lw = md["num_ent"] if one_vs_all else L
    assert pred.shape == (B, Lw) and hv.shape == (B, md["ent_emb_size"])
    # the logits are the scorer on the train-mode embedding
    E = before["ent_emb"].double().cpu().numpy()
    pb = before["pred_bias"].double().cpu().numpy()
    if one_vs_all:
        want = hv.astype(np.float64) @ E.T + pb[None, :]
    else:
        lk = batch["lookup_values"].astype(np.int64)
        want = np.einsum("bd,bld->bl", hv.astype(np.float64), E[lk]) + pb[lk]
    assert np.abs(pred - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    # ... and the loss is models.py:448-453 on them
    t = (1.0 - 0.1) * batch["e2_multi"].astype(np.float64) + 1.0 / md["num_ent"]
    s = pred.astype(np.float64)
    bce = np.maximum(s, 0) - s * t + np.log1p(np.exp(-np.abs(s)))
    assert abs(loss_f - bce.mean()) <= 2e-5 * max(1.0, abs(bce.mean()))
    # the step that follows draws the same masks and statistics: the same loss, bit for bit -- and it does update
    loss_s = float(m.train_step(batch).cpu()[0])
    assert loss_s == loss_f
    assert not torch.equal(m._tensors["ent_emb"], before["ent_emb"])
    m.close()


def test_one_vs_all_training_through_the_loader():
    """`config_nations_plain.yaml`-shaped training (plain ConvE, `num_labels` empty -> 1-vs-all labels, data.py:157-158,
    314-330; run_cpg.py:116 builds the model with use_negative_sampling=False): loader.train_dataset(num_labels=None, device=)
    -> dense e2_multi [B, |E|] built on the device -> the reference's own `session.run((loss, train_op), {is_train: True})`.
    The loss falls and the filtered MRR on the train graph ends far above its start."""
    from coper_amd.data import EvalDataset, OneVsAllTrainDataset, SyntheticKGLoader
    from coper_amd.metrics import ranking_and_hits
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("nations_cpg", ent_emb_size=40, rel_emb_size=40, emb_h=10, emb_w=4, context_rel_conv=None,
                                 context_rel_out=None, conv_num_channels=8, num_ent=60, num_rel=8)
    md.update(use_negative_sampling=False, batch_norm_train_stats=False, hidden_dropout=0.1, output_dropout=0.1,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    ld = SyntheticKGLoader("nations_plain_like", seed=1, queries=300, md=md)
    ds = ld.train_dataset(None, batch_size=64, num_labels=None, device="cuda:0")
    assert isinstance(ds, OneVsAllTrainDataset)
    s = ld.train_samples()
    p = cdata.reference_init_params(md, 3)                      # the reference's own starting point (models.py:205-214, 284-293)
    m = ConvE(md, device="cuda:0").load_parameters(p)
    # the training triples as an evaluation set: every (e1, rel, tail) with the record's other tails filtered
    n = np.diff(s["tail_indptr"])
    q = dict(e1=np.repeat(s["e1"], n), rel=np.repeat(s["rel"], n), e2=s["tail_idx"].astype(np.int64),
             filt_indptr=np.concatenate([[0], np.cumsum(np.repeat(n, n))]).astype(np.int64),
             filt_idx=np.concatenate([s["tail_idx"][s["tail_indptr"][i]:s["tail_indptr"][i + 1]] for i in range(len(n)) for _ in range(n[i])]).astype(np.int64))
    mrr0 = ranking_and_hits(m, None, EvalDataset(q, 256, md["num_ent"]), "before")[1]
    sess = m.session()
    it = iter(ds)
    losses = []
    for step in range(400):
        loss, _ = sess.run((m.loss, m.train_op), {m.is_train: True, m.input_iterator_handle: it})
        losses.append(loss)
    mrr1 = ranking_and_hits(m, None, EvalDataset(q, 256, md["num_ent"]), "after")[1]
    assert np.mean(losses[-20:]) < 0.7 * np.mean(losses[:20]), (losses[:3], losses[-3:])
    assert mrr1 > mrr0 + 0.1, (mrr0, mrr1)
    m.close()


def test_training_steps_between_streamed_evaluation_passes():
    """An evaluation stream interrupted by training steps (run_cpg.py:211-250: train, then evaluate, then train on): a registration
    made with coper_group_next and a grouping prepared ahead do not survive a training step, ranks registered with
    coper_post_i32_next leave with the next call that sorts a batch by relation (the step itself for a parameter-lookup model, the
    next evaluation pass otherwise), and the evaluation passes around the steps return what plain passes return on the weights of
    the moment."""
    from coper_amd.models import ConvE
    for case in ("cpg_linear", "lookup"):
        md = dict(cdata._COMMON)
        md.update(_CASES[case])
        md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2,
                  label_smoothing_epsilon=0.1, learning_rate=0.003)
        p0 = cdata.synthetic_params(md, seed=8, ent_std=0.1)
        m = ConvE(md, device="cuda:0", score_mode="bf16x3")
        m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
        m.train_init(seed=11)
        Q = 300
        qa, qb = cdata.synthetic_queries(md, Q, seed=5), cdata.synthetic_queries(md, Q, seed=6)
        da = {k: torch.as_tensor(np.asarray(v)).to("cuda:0") for k, v in qa.items()}
        db = {k: torch.as_tensor(np.asarray(v)).to("cuda:0") for k, v in qb.items()}

        def plain(d):
            return m.rank_pass(d["e1"], d["rel"], d["e2"], d["filt_indptr"], d["filt_idx"], want_equal=False)[0].cpu().numpy()

        host = torch.full((Q,), -1, dtype=torch.int32).pin_memory()
        ranks = torch.empty(Q, dtype=torch.int32, device="cuda:0")
        for rep in range(3):
            want_a = plain(da)
            m.group_next(db["e1"], db["rel"])                      # B is announced as the pass after the next one ...
            r, _ = m.rank_pass(da["e1"], da["rel"], da["e2"], da["filt_indptr"], da["filt_idx"], want_equal=False, out=ranks)
            m.post_next(r, host)
            m.group_next(da["e1"], da["rel"])                      # ... and one more registration that no evaluation pass will carry
            m.train_step(_batch(md, 40, 29, seed=20 + rep))        # the weights move
            torch.cuda.synchronize()
            if case == "lookup":                                   # (its step sorted its batch: the ranks left beside that launch)
                assert np.array_equal(host.numpy(), want_a), rep
            got_b, _ = m.rank_pass(db["e1"], db["rel"], db["e2"], db["filt_indptr"], db["filt_idx"], want_equal=False)
            got_b = got_b.cpu().numpy()
            assert np.array_equal(host.numpy(), want_a), (case, rep)
            assert np.array_equal(got_b, plain(db)), (case, rep)   # (on the NEW weights: nothing of the old grouping or planes was used)
            host.fill_(-1)
        m.close()


_SIDE_CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.test_gpu_train import _run_few_steps
print("RESULT " + json.dumps(_run_few_steps(%(names)r)))
"""


def _run_few_steps(names):
    """Three training steps of each case from seeded variables: the losses and every variable afterwards (as lists)."""
    from coper_amd.models import ConvE
    out = {}
    for name in names:
        md = dict(cdata._COMMON)
        md.update(_CASES[name])
        md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
                  learning_rate=0.003)
        p0 = cdata.synthetic_params(md, seed=33, ent_std=0.1)
        m = ConvE(md, device="cuda:0")
        m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
        m.train_init(seed=9)
        losses = [float(m.train_step(_batch(md, 96, 53, seed=300 + i)).cpu()[0]) for i in range(3)]
        out[name] = dict(losses=losses, variables={k: m._tensors[k].cpu().numpy().reshape(-1).astype(np.float64).tolist() for k in sorted(p0)})
        m.close()
    return out


def test_side_streams_change_the_schedule_only():
    """Round 6: a step forks the scorer's backward and the dP product onto side streams of the training state.  A fresh process with
    COPER_TRAIN_ONE_STREAM=1 runs the same steps as one chain: the same losses and variables (up to the order of the step's float
    atomics, which neither schedule fixes)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ["cpg_wide", "plain_wide", "lookup", "cpg_conv_mlp", "cpg_linear_e20k"]
    env = dict(os.environ, COPER_TRAIN_ONE_STREAM="1")
    child = subprocess.run([sys.executable, "-c", _SIDE_CHILD % dict(root=root, names=names)], env=env, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stderr[-4000:]
    one = json.loads([ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert "COPER_TRAIN_ONE_STREAM" not in os.environ
    two = _run_few_steps(names)
    for name in names:
        for a, b in zip(one[name]["losses"], two[name]["losses"]):
            assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (name, a, b)
        bias_gap = 0.0
        if "conv1_bias" in one[name]["variables"]:
            bias_gap = np.abs(np.array(one[name]["variables"]["conv1_bias"]) - np.array(two[name]["variables"]["conv1_bias"])).max()
        for k, va in one[name]["variables"].items():
            if k == "conv1_bias":      # exact gradient 0 under batch-statistics BN: its steps are rounding noise (see _train_step_case)
                continue
            va, vb = np.array(va), np.array(two[name]["variables"][k])
            tol = 1e-5 * max(1.0, np.abs(va).max()) + (bias_gap if k == "Conv1BN/moving_mean" else 0.0)
            assert np.abs(va - vb).max() <= tol, (name, k, np.abs(va - vb).max(), tol)
