"""One rank of tests/test_gpu_train_sync_parallel.py: a fresh process that joins a process group, trains a replica through
coper_amd.parallel.DataParallelTrainer(sync_bn=True) in deterministic mode and writes what it holds after every update to an .npz
file.  Not a test module."""
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
    ap.add_argument("--form", default="sampled")
    ap.add_argument("--updates", type=int, default=1)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import numpy as np
    import torch
    import torch.distributed as dist
    from coper_amd import data as cdata
    from coper_amd.models import ConvE
    from coper_amd.parallel import DataParallelTrainer, shard_batch
    from tests import split_common as S
    from tests.parallel_child import global_batches, snapshot

    dev = a.rank if a.backend == "nccl" else 0          # gloo: the ranks share cuda:0
    torch.cuda.set_device(dev)
    device = torch.device("cuda", dev)
    kw = dict(device_id=device) if a.backend == "nccl" else {}
    dist.init_process_group(a.backend, init_method="tcp://127.0.0.1:%d" % a.port, rank=a.rank, world_size=a.world,
                            timeout=datetime.timedelta(seconds=60), **kw)
    md = S.md_for(a.case)
    # (every rank but 0 starts from OTHER variables: the trainer's broadcast makes them rank 0's)
    p0 = cdata.synthetic_params(md, seed=21 + a.rank, ent_std=0.1)
    m = ConvE(md, device=device)
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=S.SEED, clip_norm=S.CLIP, deterministic=True)      # (one seed: the masks follow the sample's place in the whole batch)
    tr = DataParallelTrainer(m, sync_bn=True)
    assert tr.world == a.world and tr.rank == a.rank and tr.sync_bn
    out = {"layout": np.array(json.dumps(tr.layout))}
    for u in range(a.updates):
        (g,) = global_batches(md, a.form, u, 1)
        loss = tr.step(shard_batch(g, a.rank, a.world))
        out["u%d/loss" % u] = loss.cpu().numpy().copy()
        out["u%d/flat" % u] = tr.flat.cpu().numpy().copy()          # the all-reduced SUM of the gradients
        out["u%d/norm" % u] = np.float64(m.train_grad("ent_emb")[1])
        out["u%d/phase" % u] = np.int64(m.train_sync_phase)
        snapshot(m, out, "u%d" % u)
    np.savez(a.out, **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
