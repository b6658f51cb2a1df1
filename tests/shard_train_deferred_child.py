"""One rank of tests/test_gpu_train_sharded_deferred.py: a fresh process that joins a process group, trains its shard of the entity
table in the deferred-rows mode through coper_amd.parallel.EntityShardedTrainer(model, group) and writes what it
holds to an .npz file (tests/shard_train_sampled_child.py is the mode-off twin).  Also the home of what both sides build: the models in
the mode, the planted slots and the batches whose ids leave rows behind.  Not a test module."""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TABLES = ("ent_emb", "pred_bias")
# the residues (id % 4) a step's batch draws its ids from: residue 1 is named again one update behind (step 2), residue 2 two behind
# (step 2), residue 3 three behind (step 3); residue 0 in every step; later steps repeat the schedule
SCHEDULE = ((0, 1), (0,), (0, 1, 2), (0, 1, 2, 3))


def planted_slots(md, seed=9):
    """The slots of tests/test_gpu_train_rows_edges.py::_planted for every row of both tables: m ~ N(0, 1e-3), v ~ U(1e-9, 1e-5),
    v_hat = v U(1, 3), float32 -- a row that misses one update moves p by about 1e-3."""
    rng = np.random.default_rng(seed)
    out = {}
    for leaf, shape in (("ent_emb", (md["num_ent"], md["ent_emb_size"])), ("pred_bias", (md["num_ent"],))):
        mm = rng.normal(0, 1e-3, shape).astype(np.float32)
        vv = rng.uniform(1e-9, 1e-5, shape).astype(np.float32)
        hh = (vv * rng.uniform(1.0, 3.0, shape)).astype(np.float32)
        out[leaf] = (mm, vv, hh)
    return out


def pool_batch(md, B, L, seed, pool, out_of_range=True):
    """A sampled batch whose e1 and lookup ids are drawn from `pool` (an id array): e1 names one id twice, one lookup row carries an id
    twice, one id is the e1 and a lookup entry of the same sample; with out_of_range (pool must hold id 0) row 3 starts with four ids
    outside [0, E), which count as row 0."""
    rng = np.random.default_rng(seed)
    pool = np.asarray(pool, np.int64)
    e1 = pool[rng.integers(0, len(pool), B)]
    lookup = pool[rng.integers(0, len(pool), (B, L))]
    labels = np.zeros((B, L), np.float32)
    labels[:, 0] = 1.0
    labels[rng.random((B, L)) < 0.05] = 1.0
    e1[1] = e1[0]
    lookup[2, L - 1] = lookup[2, L - 2]
    e1[4 % B] = lookup[4 % B, 1]
    if out_of_range:
        assert 0 in pool
        E = md["num_ent"]
        lookup[3 % B, :4] = [-1, E, E + 5, -7]
    return dict(e1=e1.astype(np.int64), rel=rng.integers(0, md["num_rel"], B).astype(np.int64), lookup_values=lookup.astype(np.int32),
                e2_multi=labels)


def schedule_batch(md, B, L, step):
    """The batch of step `step` of SCHEDULE: ids with id % 4 in the step's residues."""
    ids = np.arange(md["num_ent"])
    return pool_batch(md, B, L, 4100 + step, ids[np.isin(ids % 4, SCHEDULE[step % 4])])


def named_rows(batch, E):
    """The unique clamped ids of a batch (what a step lists) and those of its e1 alone."""
    e1 = np.asarray(batch["e1"], np.int64).copy()
    lk = np.asarray(batch["lookup_values"], np.int64).reshape(-1).copy()
    for a in (e1, lk):
        a[(a < 0) | (a >= E)] = 0
    return np.unique(np.concatenate([e1, lk])), np.unique(e1)


def deferred_shard(md, p0, lo, hi, clip, deferred=True, planted=None, device="cuda:0", chunk=128, seed=5):
    """A shard model in the mode (or, deferred=False, the mode-off sharded state of tests/shard_train_common.py::shard_model), with the
    planted slots of its own rows."""
    import torch
    from coper_amd.models import ConvE
    m = ConvE(md, device=device, shard=(lo, hi))
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=seed, clip_norm=clip, deterministic=True, entity_sharded=True, deferred_rows=deferred, one_vs_all_chunk=chunk)
    assert m.train_sharded == 1 and m.train_rows_deferred == (1 if deferred else 0)
    if planted is not None:
        m.load_optimizer_state({leaf: tuple(a[lo:hi] for a in parts) for leaf, parts in planted.items()})
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--case", required=True)
    ap.add_argument("--num-ent", type=int, required=True)
    ap.add_argument("--bounds", required=True)            # JSON: [[lo, hi], ...] in rank order
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--labels", type=int, default=30)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--clip", type=float, required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    from coper_amd import data as cdata
    from coper_amd.parallel import EntityShardedTrainer
    from tests import shard_train_common as SC

    dev = a.rank if a.backend == "nccl" else 0          # gloo: the ranks share cuda:0
    torch.cuda.set_device(dev)
    device = torch.device("cuda", dev)
    kw = dict(device_id=device) if a.backend == "nccl" else {}
    dist.init_process_group(a.backend, init_method="tcp://127.0.0.1:%d" % a.port, rank=a.rank, world_size=a.world,
                            timeout=datetime.timedelta(seconds=60), **kw)
    md = SC.md_for(a.case, a.num_ent)
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    lo, hi = json.loads(a.bounds)[a.rank]
    m = deferred_shard(md, p0, lo, hi, a.clip, planted=planted_slots(md), device=device)
    tr = EntityShardedTrainer(m)
    assert tr.world == a.world and tr.rank == a.rank
    out = {}
    for step in range(a.steps):
        loss = tr.step(schedule_batch(md, a.batch, a.labels, step))
        out["s%d/loss" % step] = loss.cpu().numpy().copy()
        out["s%d/norm" % step] = np.float64(m.train_grad("pred_bias")[1])
    for k, v in m.train_row_stats().items():
        out["stats/" + k] = np.int64(v)
    out["updates"] = np.int64(m.train_rows_updates)
    tr.sync_rows()
    SC.snapshot([m], out, "end/")
    np.savez(a.out, **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
