"""One rank of tests/test_gpu_train_sharded_sampled.py: a fresh process that joins a process group, trains its shard of the entity table
on SAMPLED batches through coper_amd.parallel.EntityShardedTrainer(model, group) and writes what it holds after every step to an .npz
file (tests/shard_train_child.py is the 1-vs-all twin).  Also the home of the sampled edge batch both sides draw.  Not a test module."""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def sampled_edge_batch(md, B, L, step, edges):
    """e1 / rel [B] as tests/shard_train_common.py::edge_batch draws and patches them (e1 on both sides of every bound, one id twice),
    lookup_values int32 [B, L] of global ids and e2_multi [B, L]: column 0 positive, 5 % more.  Row 0 names `edges` (both sides of
    every shard bound, the table's first and last row); rows 1 and 2 are one segment each (a whole sample on the first / the last
    row); row 3 starts with four ids outside [0, E), which count as row 0; the last column is row 7 in every sample."""
    E, R = md["num_ent"], md["num_rel"]
    rng = np.random.default_rng(900 + step)
    e1, rel = rng.integers(0, E, B), rng.integers(0, R, B)
    inner = [e for e in edges if 0 < e < E - 1]
    e1[:len(inner)] = inner
    e1[len(inner)] = e1[len(inner) + 1] = inner[0] + 1
    lookup = rng.integers(0, E, (B, L))
    labels = np.zeros((B, L), np.float32)
    labels[:, 0] = 1.0
    labels[rng.random((B, L)) < 0.05] = 1.0
    lookup[0, :len(edges)] = edges
    lookup[1, :] = edges[0]
    lookup[2, :] = edges[-1]
    lookup[3, :4] = [-1, E, E + 5, -7]
    lookup[:, L - 1] = 7
    return dict(e1=e1.astype(np.int64), rel=rel.astype(np.int64), lookup_values=lookup.astype(np.int32), e2_multi=labels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--case", required=True)
    ap.add_argument("--num-ent", type=int, required=True)
    ap.add_argument("--bounds", required=True)            # JSON: [[lo, hi], ...] in rank order
    ap.add_argument("--edges", required=True)             # JSON: the ids of sampled_edge_batch's row 0
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--labels", type=int, default=30)
    ap.add_argument("--steps", type=int, default=2)
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
    m = SC.shard_model(md, p0, lo, hi, a.clip, device=device)
    tr = EntityShardedTrainer(m)
    assert tr.world == a.world and tr.rank == a.rank
    out = {}
    for step in range(a.steps):
        loss = tr.step(sampled_edge_batch(md, a.batch, a.labels, step, tuple(json.loads(a.edges))))
        out["s%d/loss" % step] = loss.cpu().numpy().copy()
        out["s%d/norm" % step] = np.float64(m.train_grad("pred_bias")[1])
        SC.snapshot([m], out, "s%d/" % step)
    np.savez(a.out, **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
