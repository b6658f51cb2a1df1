"""GPU tests of data-parallel training (coper_amd/parallel.py: DataParallelTrainer).

The ranks are fresh child processes of the test (tests/parallel_child.py), started with subprocess.Popen in the environment
tests/test_gpu_multirank.py gives its ranks.  With fewer GPUs than ranks they share cuda:0 and talk over gloo -- a correctness run:
at most 4 ranks, 5 processes with the GPU open.  If a rank exits non-zero the others are terminated and the test fails; nothing is
started again.  The oracle and the bounds are those of tests/test_gpu_train_split.py (tests/split_common.py)."""
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
        cmd = [sys.executable, os.path.join(ROOT, "tests", "parallel_child.py"), "--rank", str(r), "--world", str(world), "--port", str(port),
               "--backend", backend, "--out", str(tmp_path / ("rank%d.npz" % r))]
        for k, v in args.items():
            cmd += ["--" + k.replace("_", "-"), json.dumps(v) if isinstance(v, dict) else str(v)]
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


_NO_DROPOUT = dict(hidden_dropout=0.0, output_dropout=0.0, context_rel_dropout=0.0)


@pytest.mark.parametrize("name,form", [("cpg_linear", "sampled"), ("plain", "dense")])
def test_two_ranks_stay_equal_and_equal_two_micro_batches(tmp_path, name, form):
    """World 2, deterministic mode, dropout 0, batch statistics on, three updates of a global B = 48.  Both ranks hold identical bytes in
    every variable, moving statistic and slot; the trainable variables and the slots equal, byte for byte, a single process that takes the
    two shards as two micro-batches (a + b has one order).  The moving statistics are not compared with the single process: it moves them
    twice per update, the ranks once each and average."""
    from coper_amd.models import ConvE
    from coper_amd.parallel import DataParallelTrainer, shard_batch
    ranks = _run_ranks(tmp_path, 2, case=name, form=form, over=_NO_DROPOUT, updates=3, deterministic=1)
    assert sorted(ranks[0]) == sorted(ranks[1])
    for k in ranks[0]:
        assert ranks[0][k].tobytes() == ranks[1][k].tobytes(), k
    # writing the averaged moving statistics did not cost the step its carried maximum of the dense weights
    assert all(int(r["u%d/wmax" % u]) == 1 for r in ranks for u in range(3))
    md = S.md_for(name, **_NO_DROPOUT)
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=S.SEED, clip_norm=S.CLIP, deterministic=True)
    tr = DataParallelTrainer(m, micro_batches=2)
    for u in range(3):
        (g,) = global_batches(md, form, u, 1)
        tr.step([shard_batch(g, 0, 2), shard_batch(g, 1, 2)])
        assert tr.flat.cpu().numpy().tobytes() == ranks[0]["u%d/flat" % u].tobytes(), u
        for leaf in m.trainable_leaves():
            assert m._tensors[leaf].cpu().numpy().tobytes() == ranks[0]["u%d/var/%s" % (u, leaf)].tobytes(), (u, leaf)
    slots, powers = m.optimizer_state()
    for leaf, parts in slots.items():
        for i, part in enumerate(parts):
            assert np.array(part).tobytes() == ranks[0]["u2/slot%d/%s" % (i, leaf)].tobytes(), (leaf, i)
    assert powers["beta1_power"] == float(ranks[0]["u2/power/beta1_power"])
    m.close()


def _against_oracle(ranks, name, form, world, micro, updates):
    """Rank 0's gradients, norm and variables after every update against the oracle: the mean of the world * micro shard gradients, each
    with its rank's own masks (seed + rank, that rank's dropout counter) and its own batch statistics, through one AMSGrad.step; the
    moving statistics each rank moved, averaged.  From the second update on the oracle restarts from rank 0's variables, so every update
    is held to the step-0 bounds."""
    from coper_amd.parallel import shard_batch
    md = S.md_for(name)
    ref, opt = S.new_oracle(md, cdata.synthetic_params(md, seed=21, ent_std=0.1))
    stats = [k for k in ref if k.endswith(("moving_mean", "moving_variance"))]
    r0 = ranks[0]
    for u in range(updates):
        if u > 0:
            for k in ref:
                ref[k] = r0["u%d/var/%s" % (u - 1, k)].reshape(np.shape(ref[k])).astype(np.float64)
        grads, losses, moved = [], [], []
        batches = global_batches(md, form, u, micro)
        for r in range(world):
            ref_r = dict(ref)
            for i, g in enumerate(batches):
                lo, gr = S.oracle_backward(ref_r, md, shard_batch(g, r, world), S.SEED + r, u * micro + i)
                grads.append(gr)
                losses.append(lo)
            moved.append({k: ref_r[k] for k in stats})
        for k in stats:
            ref[k] = sum(mv[k] for mv in moved) / float(world)
        mean_o, gn_o = S.oracle_update(ref, opt, grads)
        loss = float(r0["u%d/loss" % u][0])
        assert abs(loss - np.mean(losses)) < 2e-5 * max(1.0, abs(np.mean(losses))), (u, loss, np.mean(losses))
        layout = {k: tuple(v) for k, v in json.loads(str(r0["layout"])).items()}
        mean_dev = S.flat_slices(r0["u%d/flat" % u] * np.float32(1.0 / (world * micro)), layout)
        dg = S.check_grads(mean_dev, mean_o, gn_o, "update %d" % u)
        gn = float(r0["u%d/norm" % u])
        assert abs(gn - gn_o) < 1e-4 * gn_o, (u, gn, gn_o)
        S.check_variables(md, {k: r0["u%d/var/%s" % (u, k)] for k in ref}, ref, dg, "update %d" % u)


def test_two_ranks_with_their_own_dropout_masks_match_the_oracle(tmp_path):
    """World 2, dropout on, seeds s + rank, one update: rank 0's variables against the mean of the two shard gradients."""
    ranks = _run_ranks(tmp_path, 2, case="cpg_linear", form="sampled", updates=1, seed_per_rank=1)
    _against_oracle(ranks, "cpg_linear", "sampled", 2, 1, 1)


def test_four_ranks_two_micro_batches(tmp_path):
    """World 4, micro_batches = 2, two updates: the four replicas are byte-identical, rank 0 matches the oracle."""
    ranks = _run_ranks(tmp_path, 4, case="cpg_mlp_bn", form="sampled", updates=2, micro=2, seed_per_rank=1)
    for r in range(1, 4):
        for k in ranks[0]:
            if "/var/" in k or "/slot" in k or "/power/" in k or k.endswith("/flat"):
                assert ranks[0][k].tobytes() == ranks[r][k].tobytes(), (r, k)
    _against_oracle(ranks, "cpg_mlp_bn", "sampled", 4, 2, 2)
