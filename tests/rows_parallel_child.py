"""One rank of tests/test_gpu_train_rows_parallel.py: a fresh process that joins a process group, trains a replica in the deferred-rows
mode through coper_amd.parallel.DataParallelTrainer's sparse route and writes what it holds after every update to an .npz file.  Not a
test module."""
import argparse
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GLOBAL_B, PRE_STEPS = 16, 2


def global_batches(md, update, micro):
    """The `micro` GLOBAL batches (B = 16, L = 12, |E| = 257) of update `update`: every rank and the test build the same ones.  Ids
    outside [0, E) in both halves: row 0, as the step's kernels clamp them."""
    from tests.test_gpu_train_rows import E, L, _batch_below
    out = []
    for i in range(micro):
        b = _batch_below(md, E, GLOBAL_B, L, 700 + update * micro + i)
        b["lookup_values"][0, 0] = E + 5
        b["lookup_values"][GLOBAL_B - 1, 1] = -3
        out.append(b)
    return out


def pre_batches(md):
    """What rank 0 trains on BEFORE the trainer exists: ids below 100, so that the rows above are behind when its state is broadcast."""
    from tests.test_gpu_train_rows import B, L, _batch_below
    return [_batch_below(md, 100, B, L, 650 + i) for i in range(PRE_STEPS)]


def snapshot(m, out, tag):
    import numpy as np
    slots, powers = m.optimizer_state()      # (syncs the rows: the raw tables read below are current)
    for k, v in m._tensors.items():
        out["%s/var/%s" % (tag, k)] = v.cpu().numpy().copy()
    for leaf, parts in slots.items():
        for i, part in enumerate(parts):
            out["%s/slot%d/%s" % (tag, i, leaf)] = np.array(part)
    for k, v in powers.items():
        out["%s/power/%s" % (tag, k)] = np.float64(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--case", required=True)
    ap.add_argument("--micro", type=int, default=2)
    ap.add_argument("--updates", type=int, default=2)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import json
    import numpy as np
    import torch
    import torch.distributed as dist
    from coper_amd import data as cdata
    from coper_amd.models import ConvE
    from coper_amd.parallel import DataParallelTrainer, shard_batch
    from tests import split_common as S
    from tests.test_gpu_train_rows import _md

    dev = a.rank if a.backend == "nccl" else 0          # gloo: the ranks share cuda:0
    torch.cuda.set_device(dev)
    device = torch.device("cuda", dev)
    kw = dict(device_id=device) if a.backend == "nccl" else {}
    dist.init_process_group(a.backend, init_method="tcp://127.0.0.1:%d" % a.port, rank=a.rank, world_size=a.world,
                            timeout=datetime.timedelta(seconds=60), **kw)
    md = _md(a.case)
    # (every rank but 0 starts from OTHER variables: the trainer's broadcast makes them rank 0's)
    p0 = cdata.synthetic_params(md, seed=21 + a.rank, ent_std=0.1)
    m = ConvE(md, device=device)
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=S.SEED, clip_norm=S.CLIP, deferred_rows=True)
    if a.rank == 0:
        for b in pre_batches(md):
            m.train_step(b)
    out = {"pre/rows_behind": np.int64(m.train_row_stats()["rows_behind"])}
    tr = DataParallelTrainer(m, micro_batches=a.micro)
    assert tr.world == a.world and tr.rank == a.rank and tr.sparse
    out["layout"] = np.array(json.dumps(tr.layout))
    snapshot(m, out, "init")
    d = md["ent_emb_size"]
    for u in range(a.updates):
        local = [shard_batch(b, a.rank, a.world) for b in global_batches(md, u, a.micro)]
        loss = tr.step(local)
        out["u%d/loss" % u] = loss.cpu().numpy().copy()
        out["u%d/small" % u] = tr.flat.cpu().numpy().copy()          # the all-reduced SUM of the small gradients
        out["u%d/ids" % u] = tr.gathered[0].cpu().numpy().copy()     # [W, M, mx]
        out["u%d/vals" % u] = tr.gathered[1].cpu().numpy().copy()    # [W, M, mx, rs]
        out["u%d/rows_last_step" % u] = np.int64(m.train_row_stats()["rows_last_step"])
        for leaf in ("ent_emb", "pred_bias"):                        # the SUM of the imported blocks, as the dense buffers hold it
            g, gn = m.train_grad(leaf)
            out["u%d/grad/%s" % (u, leaf)] = g.cpu().numpy().copy()
        out["u%d/norm" % u] = np.float64(gn)
        snapshot(m, out, "u%d" % u)
    np.savez(a.out, **out)
    m.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
