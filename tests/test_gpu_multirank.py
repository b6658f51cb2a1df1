"""GPU: N > 1 ranks of the HIP scorer, started the way the driver starts `bench.py` -- from a plain shell.

`python bench.py --gpus 2` (no WORLD_SIZE) starts its two ranks itself as fresh child processes (bench.py: self_launch).
On a box with one GPU the ranks share it and talk over gloo (`--dist-backend gloo`); with two or more GPUs they get one
each and talk over RCCL.  Either way every rank runs the real kernels on its own shard:
  * main line: query-sharded, every rank its own 20,480 queries on a replicated model (weak scaling);
  * `scale` block: BASELINE.json configs[4] (10 M entities x 256), entity-sharded -- each rank holds a 5 M-row shard, the
    encoder is split by relation, the per-shard (counts, top-10) records are exchanged in the one all-gather -- and the
    ranks must equal the single-GPU ranks of the same KG bit for bit (`ranks_independent_of_world`, SHA-1 of the ranks
    against the committed single-GPU value)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(extra, timeout=600, world=2):
    import torch
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--dist-backend", backend, "--steps", "3",
                          "--warmup", "1", "--no-cpu-baseline", "--launch-timeout", str(timeout - 60)] + extra, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), backend


def test_bench_two_ranks_from_a_plain_shell():
    from bench import SCALE_EXPECTED
    line, backend = _run_bench(["--full"])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["value"] > 0
    assert line["config"]["parallelism"] == "query-sharded x2"
    sc = line["scale"]
    assert sc["n_gpus"] == 2 and sc["config"]["parallelism"].startswith("entity-sharded x2 (5000000 rows per rank)")
    assert sc["ranks_independent_of_world"] is True
    assert sc["ranks_sha1"] == SCALE_EXPECTED["ranks_sha1"]
    assert abs(sc["mean_rank"] - SCALE_EXPECTED["mean_rank"]) < 1e-6


def test_bench_two_ranks_entity_sharded_main_line():
    """The entity-sharded path as the main line on a small KG (WN18RR-shaped), top-10 exchanged: its ranks are those of the
    one-rank run of the same command (mean rank / MRR carried by the line)."""
    two, _ = _run_bench(["--workload", "wn18rr_cpg", "--mode", "entity", "--topk", "10", "--no-extras"], timeout=420)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "wn18rr_cpg", "--mode", "entity", "--topk", "10",
                          "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-extras"], env=env, capture_output=True, text=True,
                         timeout=420)
    assert out.returncode == 0, out.stderr[-4000:]
    one = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["config"]["mean_rank"] == one["config"]["mean_rank"] and two["config"]["mrr"] == one["config"]["mrr"]


def test_bench_two_ranks_three_times_back_to_back():
    """round 3 saw ONE two-rank run hang in a full-suite pass (never reproduced; the one latent deadlock found
    since -- rank 0 blocking on a stdout pipe nobody drained -- is gone: bench.py's self_launch reads a file).  Three launches
    in a row, each bounded by --launch-timeout, each with the ranks of the others."""
    ranks = []
    for _ in range(3):
        line, _ = _run_bench(["--no-extras"], timeout=300)
        assert line["n_gpus"] == 2 and line["value"] > 0
        ranks.append((line["config"]["mean_rank"], line["config"]["mrr"]))
    assert ranks[0] == ranks[1] == ranks[2]


@pytest.mark.parametrize("world", [4, 8])
def test_bench_scale_block_at_the_target_world_size(world):
    """the entity-sharded path at north_star's own world size with the REAL kernels.  On a one-GPU box the
    ranks share the GPU and talk over gloo (8 x (a 1.25 M-row shard's planes + the rank's W_r cache) fits 288 GB); with >= `world`
    GPUs they get one each over RCCL.  1.25 M-row (2.5 M-row) shards, the `rel mod world` encoder split, k_band_exact<3> on shards,
    the 8-row (4-row) all-gather layouts -- and the ranks of every chunk must be the single-GPU ranks bit for bit (SHA-1)."""
    from bench import SCALE_EXPECTED
    # (world 4 also with the side stream's collectives on a communicator of their own: the opt-in form)
    line, backend = _run_bench(["--full"] + (["--scale-side-communicator"] if world == 4 else []), timeout=900, world=world)
    assert line["n_gpus"] == world and line["value"] > 0
    assert line["config"]["parallelism"] == "query-sharded x%d" % world
    sc = line["scale"]
    assert sc["n_gpus"] == world
    assert sc["config"]["parallelism"].startswith("entity-sharded x%d (%d rows per rank)" % (world, 10_000_000 // world))
    assert sc["ranks_independent_of_world"] is True
    assert sc["ranks_sha1"] == SCALE_EXPECTED["ranks_sha1"]
    assert abs(sc["mean_rank"] - SCALE_EXPECTED["mean_rank"]) < 1e-6
