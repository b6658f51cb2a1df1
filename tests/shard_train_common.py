"""Shared by tests/test_gpu_train_sharded.py and its rank processes (tests/shard_train_child.py): the models, the batches and the
snapshot of an entity-sharded training run (coper_amd.parallel.EntityShardedTrainer).  Not a test module.

Model dimensions are those of tests/test_gpu_train_csr.py's _DIMS with another entity count; the descriptors' training settings
(batch statistics, dropout 0.3 / 0.2, label smoothing) are that file's."""
import numpy as np

from tests.test_gpu_train_csr import _md, _table

SEED = 5
CHUNK = 128
# the shards of E = 300 at one_vs_all_chunk = 128: every shard is exactly one chunk, the last one ragged
E300 = 300
BOUNDS300 = ((0, 128), (128, 256), (256, 300))
# the float64 oracle's global norm of these batches is 0.07 .. 0.16 (the loss is a mean over B * E logits): far below CLIP_OFF, far
# above CLIP_ACTIVE.  The tests assert both relations on the recorded / the oracle's norm, so that a change of the batches cannot
# make either case vacuous.
CLIP_OFF = 5.0
CLIP_ACTIVE = 0.02


def md_for(name, num_ent, **over):
    md = _md(name)
    md.update(num_ent=int(num_ent))
    md.update(over)
    return md


def edge_batch(md, B, step, edges):
    """e1 / rel [B] and sparse labels over a table of 20 rows: row 0 holds the columns `edges` (both sides of every shard bound, the
    table's first and last column), row 1 is empty; e1 names the entities on both sides of every bound and one id twice."""
    E, R = md["num_ent"], md["num_rel"]
    rng = np.random.default_rng(700 + step)
    e1, rel = rng.integers(0, E, B), rng.integers(0, R, B)
    inner = [e for e in edges if 0 < e < E - 1]
    e1[:len(inner)] = inner
    e1[len(inner)] = e1[len(inner) + 1] = inner[0] + 1      # one id twice, beside a bound
    rows = [np.nonzero(rng.random(E) < 0.05)[0] for _ in range(20)]
    rows[0] = list(edges)
    rows[1] = []
    indptr, idx = _table(rows)
    lab_row = rng.integers(0, 20, B)
    lab_row[:4] = [0, 1, 0, 7]
    return dict(e1=e1.astype(np.int64), rel=rel.astype(np.int64), lab_indptr=indptr, lab_idx=idx, lab_row=lab_row.astype(np.int64))


def batch300(md, step, B=48):
    return edge_batch(md, B, step, (0, 127, 128, 255, 256, 299))


def host_params(p0):
    return {k: np.array(v, np.float32) for k, v in p0.items()}


def single_model(md, p0, clip, chunk=CHUNK, device="cuda:0"):
    """The deterministic whole-table handle: train_step on sparse labels walks chunks of `chunk` columns."""
    import torch
    from coper_amd.models import ConvE
    m = ConvE(md, device=device)
    m.load_parameters({k: torch.as_tensor(v) for k, v in host_params(p0).items()})
    m.train_init(seed=SEED, clip_norm=clip, deterministic=True, one_vs_all_chunk=chunk)
    return m


def shard_model(md, p0, lo, hi, clip, chunk=CHUNK, device="cuda:0", score_mode="f32"):
    import torch
    from coper_amd.models import ConvE
    m = ConvE(md, device=device, shard=(lo, hi), score_mode=score_mode)
    m.load_parameters({k: torch.as_tensor(v) for k, v in host_params(p0).items()})      # (ent_emb / pred_bias: sliced to the shard)
    m.train_init(seed=SEED, clip_norm=clip, deterministic=True, entity_sharded=True, one_vs_all_chunk=chunk)
    return m


TABLES = ("ent_emb", "pred_bias")


def snapshot(models, out=None, tag=""):
    """Everything a run holds, as host arrays: variables and BN statistics, slots, powers -- the tables' rows concatenated in the
    order of `models`, every replicated leaf from models[0]."""
    out = {} if out is None else out
    states = [m.optimizer_state() for m in models]
    for k in models[0]._tensors:
        ms = models if k in TABLES else models[:1]
        out["%svar/%s" % (tag, k)] = np.concatenate([m._tensors[k].cpu().numpy() for m in ms])
    for leaf in states[0][0]:
        ss = states if leaf in TABLES else states[:1]
        for i in range(3):
            out["%sslot%d/%s" % (tag, i, leaf)] = np.concatenate([np.array(s[0][leaf][i]) for s in ss])
    for k, v in states[0][1].items():
        out["%spower/%s" % (tag, k)] = np.float64(v)
    return out


def replicated_equal(models):
    """Asserts that every replicated leaf and its slots are byte-identical on all models."""
    states = [m.optimizer_state() for m in models]
    for k in models[0]._tensors:
        if k in TABLES:
            continue
        for m in models[1:]:
            assert m._tensors[k].cpu().numpy().tobytes() == models[0]._tensors[k].cpu().numpy().tobytes(), k
    for leaf in states[0][0]:
        if leaf in TABLES:
            continue
        for s in states[1:]:
            for i in range(3):
                assert np.array(s[0][leaf][i]).tobytes() == np.array(states[0][0][leaf][i]).tobytes(), (leaf, i)
    for s in states[1:]:
        assert s[1] == states[0][1]


def same_bits(a, b, what=""):
    assert sorted(a) == sorted(b), (sorted(set(a) ^ set(b)), what)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)
