"""One rank of tests/test_gpu_train_sharded_forward.py: a fresh process that joins a process group, makes one sampled step on its shard of
the entity table through coper_amd.parallel.EntityShardedTrainer(model, group), then LOOKS at two batches with `forward` -- a sampled
one and a sparse 1-vs-all one -- and writes what it saw to an .npz file.  Not a test module."""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(tr, md, B, L, edges):
    """What both sides do: one step, two forwards -> {name: host array}; the 1-vs-all blocks as a list in the in-process form."""
    from tests import shard_train_common as SC
    from tests.shard_train_sampled_child import sampled_edge_batch
    out = {}
    out["step/loss"] = tr.step(sampled_edge_batch(md, B, L, 0, edges)).cpu().numpy().copy()
    loss, pred, hv = tr.forward(sampled_edge_batch(md, B, L, 1, edges), True, True)
    out["sampled/loss"], out["sampled/pred"], out["sampled/h"] = loss.cpu().numpy().copy(), pred.cpu().numpy().copy(), hv.cpu().numpy().copy()
    loss, pred, _ = tr.forward(SC.edge_batch(md, B, 2, edges), True)
    out["csr/loss"] = loss.cpu().numpy().copy()
    out["csr/pred"] = [p.cpu().numpy().copy() for p in pred] if isinstance(pred, list) else pred.cpu().numpy().copy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--case", required=True)
    ap.add_argument("--num-ent", type=int, required=True)
    ap.add_argument("--bounds", required=True)            # JSON: [[lo, hi], ...] in rank order
    ap.add_argument("--edges", required=True)             # JSON: the ids of the edge batches' row 0
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--labels", type=int, default=30)
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
    np.savez(a.out, **run(tr, md, a.batch, a.labels, tuple(json.loads(a.edges))))
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
