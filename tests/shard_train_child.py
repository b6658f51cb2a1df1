"""One rank of tests/test_gpu_train_sharded.py: a fresh process that joins a process group, trains its shard of the entity table
through coper_amd.parallel.EntityShardedTrainer(model, group) and writes what it holds after every step to an .npz file; with
--rank-queries it then prepares the shard and ranks a query chunk through coper_amd.sharding.EntityShardedRanker.  Not a test
module."""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--case", required=True)
    ap.add_argument("--num-ent", type=int, required=True)
    ap.add_argument("--bounds", required=True)            # JSON: [[lo, hi], ...] in rank order
    ap.add_argument("--edges", required=True)             # JSON: the label columns of tests/shard_train_common.py::edge_batch
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--clip", type=float, required=True)
    ap.add_argument("--score-mode", default="f32")
    ap.add_argument("--rank-queries", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import numpy as np
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
    m = SC.shard_model(md, p0, lo, hi, a.clip, device=device, score_mode=a.score_mode)
    tr = EntityShardedTrainer(m)
    assert tr.world == a.world and tr.rank == a.rank
    out = {}
    for step in range(a.steps):
        loss = tr.step(SC.edge_batch(md, 48, step, tuple(json.loads(a.edges))))
        out["s%d/loss" % step] = loss.cpu().numpy().copy()
        out["s%d/norm" % step] = np.float64(m.train_grad("pred_bias")[1])
        SC.snapshot([m], out, "s%d/" % step)
    if a.rank_queries:
        from coper_amd.sharding import EntityShardedRanker
        q = cdata.synthetic_queries(md, a.rank_queries, seed=3)
        er = EntityShardedRanker(m)      # (bf16x3: the ranks agree on the trained table's maximum here, before the shards are prepared)
        m.prepare()
        ranks, ne = er.rank({k: q[k] for k in ("e1", "rel", "e2", "filt_indptr", "filt_idx")})
        out["ranks"], out["n_equal"] = ranks.cpu().numpy().copy(), ne.cpu().numpy().copy()
    np.savez(a.out, **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
