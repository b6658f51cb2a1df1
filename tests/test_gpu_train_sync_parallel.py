"""GPU test of data-parallel training with synchronised batch statistics (coper_amd/parallel.py: DataParallelTrainer(sync_bn=True);
DESIGN.md 6.13).

The ranks are fresh child processes of the test (tests/sync_bn_child.py), started with subprocess.Popen in the environment
tests/test_gpu_multirank.py gives its ranks.  With fewer GPUs than ranks they share cuda:0 and talk over gloo -- a correctness run:
2 ranks, 3 processes with the GPU open.  If a rank exits non-zero the others are terminated and the test fails; nothing is started
again.  The oracle and the bounds are those of tests/split_common.py."""
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

from coper_amd import data as cdata
from tests import split_common as S
from tests.parallel_child import global_batches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIMIT = 150.0      # seconds for all ranks of one run (init_process_group itself gives up after 60)


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
        cmd = [sys.executable, os.path.join(ROOT, "tests", "sync_bn_child.py"), "--rank", str(r), "--world", str(world), "--port", str(port),
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


def test_two_ranks_make_the_whole_batch_step_and_stay_equal(tmp_path):
    """World 2, deterministic mode, dropout on, three updates of a global B = 48: both ranks hold identical bytes in every variable,
    moving statistic (never averaged: equal by construction) and slot after every update; update 0 -- gradient, norm, variables and
    moving statistics -- is ONE step of the float64 oracle on the whole batch."""
    name, form, world, updates = "cpg_linear", "sampled", 2, 3
    ranks = _run_ranks(tmp_path, world, case=name, form=form, updates=updates)
    assert sorted(ranks[0]) == sorted(ranks[1])
    for k in ranks[0]:
        if "/var/" in k or "/slot" in k or "/power/" in k or k.endswith(("/flat", "/norm", "/phase")):
            assert ranks[0][k].tobytes() == ranks[1][k].tobytes(), k
    assert all(int(r["u%d/phase" % u]) == 0 for r in ranks for u in range(updates))
    md = S.md_for(name)
    ref, opt = S.new_oracle(md, cdata.synthetic_params(md, seed=21, ent_std=0.1))
    (g,) = global_batches(md, form, 0, 1)
    loss_o, grads_o = S.oracle_backward(ref, md, g, S.SEED, 0)
    _, gn_o = S.oracle_update(ref, opt, [grads_o])
    r0 = ranks[0]
    loss = float(r0["u0/loss"][0])
    assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (loss, loss_o)
    layout = {k: tuple(v) for k, v in json.loads(str(r0["layout"])).items()}
    dg = S.check_grads(S.flat_slices(r0["u0/flat"] * np.float32(1.0 / world), layout), grads_o, gn_o, "update 0")
    gn = float(r0["u0/norm"])
    assert abs(gn - gn_o) < 1e-4 * gn_o, (gn, gn_o)
    S.check_variables(md, {k: r0["u0/var/%s" % k] for k in ref}, ref, dg, "update 0", skip_stats=False)
