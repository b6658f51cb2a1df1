"""GPU test of data-parallel training in the deferred-rows mode (coper_amd/parallel.py: DataParallelTrainer's sparse route; DESIGN.md
6.5).  ONE run: world 2, two micro-batches, two updates, the same seed on both ranks -- 3 processes with the GPU open.

The ranks are fresh child processes (tests/rows_parallel_child.py), started and watched with the discipline of
tests/test_gpu_train_parallel.py: with fewer GPUs than ranks they share cuda:0 and talk over gloo (a correctness run); one time limit
for all ranks; if a rank exits non-zero the others are terminated and the test fails; nothing is started again."""
import json
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import split_common as S
from tests.rows_parallel_child import GLOBAL_B, PRE_STEPS, global_batches
from tests.test_gpu_train_rows import E, L, _ids, _loss_close, _md

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIMIT = 150.0      # seconds for all ranks of the run (init_process_group itself gives up after 60)
WORLD, MICRO, UPDATES = 2, 2, 2


def _run_ranks(tmp_path, world, **args):
    """Starts `world` ranks, waits for them under one time limit -> [the .npz of rank r as a dict]"""
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    procs, logs = [], []
    for r in range(world):
        cmd = [sys.executable, os.path.join(ROOT, "tests", "rows_parallel_child.py"), "--rank", str(r), "--world", str(world), "--port", str(port),
               "--backend", backend, "--out", str(tmp_path / ("rank%d.npz" % r))]
        for k, v in args.items():
            cmd += ["--" + k.replace("_", "-"), str(v)]
        logs.append(open(str(tmp_path / ("rank%d.log" % r)), "wb"))
        procs.append(subprocess.Popen(cmd, env=env, stdout=logs[-1], stderr=subprocess.STDOUT, start_new_session=True, cwd=ROOT))
    failed, t0 = None, time.time()
    try:
        live = set(range(world))
        while live and failed is None:
            time.sleep(0.05)
            if time.time() - t0 > _LIMIT:
                failed = "ranks %s still running after %d s" % (sorted(live), _LIMIT)
                break
            for r in sorted(live):
                code = procs[r].poll()
                if code is None:
                    continue
                live.discard(r)
                if code != 0:
                    failed = "rank %d exited with code %d" % (r, code)
                    break
    finally:
        for pr in procs:
            if pr.poll() is None:
                try:
                    os.killpg(pr.pid, signal.SIGTERM)
                except ProcessLookupError:
                    pass
        for pr in procs:
            try:
                pr.wait(timeout=30)
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(pr.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                pr.wait()
        for f in logs:
            f.close()
    if failed is not None:
        tails = "\n".join("--- rank %d\n%s" % (r, open(str(tmp_path / ("rank%d.log" % r)), errors="replace").read()[-3000:]) for r in range(world))
        pytest.fail(failed + "\n" + tails)
    return [dict(np.load(str(tmp_path / ("rank%d.npz" % r)))) for r in range(world)]


def test_two_ranks_two_micro_batches_in_the_mode(tmp_path):
    """Global B = 16, L = 12, |E| = 257, micro_batches = 2, two updates.  Rank 0 trains two steps alone first, so that rows are behind
    when the trainer broadcasts its state: after construction both ranks hold the same bytes (the broadcast synced first).  Per update
    both ranks against the float64 oracle of the mean of the four shard gradients (each with its own masks and, per rank, its own moving
    statistics, which are then averaged) through one AMSGrad.step, restarted from rank 0's variables as tests/test_gpu_train_parallel.py
    does: loss, gradients (check_grads), norm, variables (check_variables).  rows_last_step is the union of the four shards' clamped ids
    on both ranks; the gathered ids / vals buffers and the table gradients summed from them are byte-identical across the ranks.  Byte
    equality of the replicas' VARIABLES is not asserted: the mode's norm is summed by unordered atomics."""
    from oracle import coper_train_oracle as T
    from coper_amd.parallel import shard_batch
    name = "cpg_linear"
    ranks = _run_ranks(tmp_path, WORLD, case=name, micro=MICRO, updates=UPDATES)
    assert sorted(ranks[0]) == sorted(ranks[1])
    assert int(ranks[0]["pre/rows_behind"]) > 0 and int(ranks[1]["pre/rows_behind"]) == 0
    for k in ranks[0]:
        if k.startswith("init/") or k.endswith(("/ids", "/vals", "/small", "/rows_last_step")) or "/grad/" in k:
            assert ranks[0][k].tobytes() == ranks[1][k].tobytes(), k
    md = _md(name)
    d = md["ent_emb_size"]
    layout = {k: tuple(v) for k, v in json.loads(str(ranks[0]["layout"])).items()}
    names = T.trainable_names(md)
    for rk in ranks:
        ref = {k[len("init/var/"):]: v.astype(np.float64) for k, v in rk.items() if k.startswith("init/var/")}
        opt = T.AMSGrad(names, ref, lr=md["learning_rate"], clip=S.CLIP)
        for leaf in names:      # the optimizer state rank 0 brought along from its steps alone
            shape = np.shape(ref[leaf])
            opt.m[leaf], opt.v[leaf], opt.vh[leaf] = (rk["init/slot%d/%s" % (i, leaf)].astype(np.float64).reshape(shape) for i in range(3))
        opt.b1p, opt.b2p = float(rk["init/power/beta1_power"]), float(rk["init/power/beta2_power"])
        assert int(rk["init/power/step"]) == PRE_STEPS
        stats = [k for k in ref if k.endswith(("moving_mean", "moving_variance"))]
        for u in range(UPDATES):
            if u > 0:
                for k in ref:
                    ref[k] = rk["u%d/var/%s" % (u - 1, k)].reshape(np.shape(ref[k])).astype(np.float64)
            grads, losses, moved, union = [], [], [], []
            batches = global_batches(md, u, MICRO)
            for r in range(WORLD):
                ref_r = dict(ref)
                for i, g in enumerate(batches):
                    shard = shard_batch(g, r, WORLD)
                    lv = np.array(shard["lookup_values"])
                    lv[(lv < 0) | (lv >= E)] = 0      # (the oracle indexes: ids outside [0, E) as the step's kernels clamp them)
                    lo, gr = S.oracle_backward(ref_r, md, dict(shard, lookup_values=lv), S.SEED, PRE_STEPS + u * MICRO + i)
                    grads.append(gr)
                    losses.append(lo)
                    union.append(_ids(shard))
                moved.append({k: ref_r[k] for k in stats})
            for k in stats:
                ref[k] = sum(mv[k] for mv in moved) / float(WORLD)
            mean_o, gn_o = S.oracle_update(ref, opt, grads)
            _loss_close(float(rk["u%d/loss" % u][0]), float(np.mean(losses)))
            assert int(rk["u%d/rows_last_step" % u]) == np.unique(np.concatenate(union)).size
            inv = np.float32(1.0 / (WORLD * MICRO))
            got = S.flat_slices(rk["u%d/small" % u] * inv, layout)
            got["ent_emb"], got["pred_bias"] = rk["u%d/grad/ent_emb" % u] * inv, rk["u%d/grad/pred_bias" % u] * inv
            dg = S.check_grads(got, mean_o, gn_o, "update %d" % u)
            gn = float(rk["u%d/norm" % u])
            assert abs(gn - gn_o) < 1e-4 * gn_o, (u, gn, gn_o)
            S.check_variables(md, {k: rk["u%d/var/%s" % (u, k)] for k in ref}, ref, dg, "update %d" % u)
            # the gathered buffers: [W, M, mx] blocks whose valid rows are the shards' clamped ids, each once
            ids = rk["u%d/ids" % u]
            assert ids.shape[:2] == (WORLD, MICRO) and rk["u%d/vals" % u].shape == ids.shape + ((d + 4) & ~3,)
            for r in range(WORLD):
                for i in range(MICRO):
                    blk = ids[r, i]
                    assert np.array_equal(np.sort(blk[blk >= 0]), union[r * MICRO + i]), (u, r, i)
    assert GLOBAL_B % WORLD == 0 and L == 12 and E == 257
