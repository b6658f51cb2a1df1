#!/usr/bin/env python3
"""bench.py -- scored triples/sec (1-vs-all) of the CoPER-ConvE evaluation hot path on MI355X.

A "step" = one pass of the hot path (encode -> 1-vs-all score -> filtered rank) over one batch of
synthetic queries: the evaluation set of the workload (Q queries).

  python bench.py --gpus N --steps K --warmup W
  N > 1: either launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` (RANK /
  LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment), or from a plain shell: the process then starts the N ranks
  itself as fresh child processes (before anything here touches the GPU), relays rank 0's JSON line and exits
  non-zero when any rank fails.

The JSON line (rank 0, stdout) carries, for the default workload (BASELINE.json configs[1], FB15k-237-shaped
CoPER-ConvE, bf16x3 arithmetic; query-sharded across ranks = weak scaling):

  value / ms_per_step     the SURVEY 8(d) region: K passes, each H2D of ids + CSR filters from pinned host buffers + pass + D2H
                          of the int32 ranks to pinned host memory, barrier + synchronize on both sides, MAX over ranks (the
                          driver contract)

A plain run measures that and nothing else: set-up, untimed passes until the clocks have left their idle state (SETTLE_S),
the W warm-up passes, the K timed ones, the line.  --dump-outputs DIR then writes what the timed path handed its caller in
its last step as DIR/<name>.npy (float64; inputs are seeded, so two builds can be compared output for output).  Everything
below comes with --full (and its --no-* switches):

  resident_inputs         the same K passes with ids + CSR filters resident in HBM (round 2's headline); `timing` adds
                          median / min per pass (HIP events)
  config.f32_exact        the same pass in the fp32-exact mode; `rank_agreement`: the headline mode's ranks against the fp32
                          chain's on the SAME h (equal for every query: the exact band), against the fp32-exact mode end to
                          end, and against float64 arithmetic throughout (what the two encoders' rounding of h leaves)
  roofline                the dominant kernel against its roof (HIP events on the launch stream), other kernels
                          under all_kernels -- among them the score kernel in its HBM-bound regime
                          (`k_score_count_bf16x3@hbm`: 128 queries against this rank's shard of the 10M x 256 table)
  scale                   BASELINE.json configs[4]: the 10M-entity KG, entity-sharded across the N ranks, per-shard
                          top-10 exchanged in the one all-gather; strong scaling; run at N = 1 too.
                          Its ranks must not depend on N (checked against the committed single-GPU checksum)
  cpu_baseline            torch-CPU restatement of the reference pass (oracle/coper_oracle_torch.py), all host cores
                          and one core, rank 0 at N = 1 only

  --workload X --mode entity : any one workload as the main line, entity-sharded (strong scaling)."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md: Peak FP32 (matrix)
PEAK_HBM_GBS = 8000.0
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense bf16 / fp16 MFMA (same rate); the x3 mode spends 3 hardware MFMAs per algorithmic product

SCALE_WORKLOAD, SCALE_TOPK, HBM_REGIME_QUERIES, SCALE_CHUNKS = "synth10m_cpg", 10, 128, 4
# A plain run's untimed passes before its W warm-up passes: the device takes tens of milliseconds of load to leave its idle
# power state (0.588 ms per pass over the first 20 passes after setup, 0.549 over 100, 0.532 over 400), which --full's
# secondary measurements otherwise provide.  Seconds of back-to-back passes.
SETTLE_S = 0.5
DUMP_LIMIT_BYTES = 64 << 20
# Ranks of the `scale` pass on ONE GPU holding all 10M entities (seed 0, Q = 4096, x3 mode with the scale-invariant fp16 split
# and the exact band: round 4; entity rows ~ N(0, 0.1^2) as SURVEY 8(d) says, rounds 1 - 3 drew 0.3), measured on MI355X: every
# entity sharding of the same table must reproduce them bit for bit (integer counts summed across shards).
# (round 5: the encoder's conv moved to the matrix cores -- h moves by ~1e-7 of its magnitude, a handful of the 4,096 ranks among
# 10M entities by one place: the value below is the single-GPU pass of the round-5 arithmetic; round 4's was 41cfaa9f...)
# (round 6: the block ranks SCALE_CHUNKS distinct chunks -- seeds 0..3 -- instead of one; the SHA-1 is over the ranks of all of them in
# seed order, 16,384 queries.  Measured on one GPU holding the whole table, and at world 2 and 8 sharing one GPU: the same value.
# Chunk 0 alone is round 5's 0e327a86...)
SCALE_EXPECTED = {"ranks_sha1": "39cf592c893aa596c160c13c6d87a56796d2b7c0", "mean_rank": 4944764.270263672}


def _profile_entry(pattern, workload, Q, kernel, exact=None):
    """(value dict, path) from the newest committed rocprofv3 PMC summary (profiles/), or (None, None): a summary of this
    workload holding the kernel, or -- `exact`: a template instantiation that only one shape launches (the 10M-entity
    blocks of the default command) -- any summary holding exactly that instantiation."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), reverse=True):
        try:
            d = json.load(open(path))
        except Exception:
            continue
        if exact:
            hit = [e for e in ((exact,) if isinstance(exact, str) else exact) if e in d.get("kernels", {})]
            if hit:
                return d["kernels"][hit[0]], os.path.relpath(path, ROOT)
            continue
        if d.get("workload") != workload or d.get("queries") != Q:
            continue
        for name, v in d.get("kernels", {}).items():     # template arguments (<13>, <false>) follow the base name
            if name == kernel or name.startswith(kernel + "<"):
                return v, os.path.relpath(path, ROOT)
    return None, None


def run_train_lines(budget_s=150.0):
    """SURVEY 8(f)-1 beside the line: the training step (B = 512 queries x L = 1000 sampled entities: forward, backward, clip,
    AMSGrad) of the three shipped model shapes, each timed by `tools/bench_train.py` in a child process of its own (a fresh
    training state; this process has finished its timed regions).  Reported, not part of `value`.  Skipped under a profiler
    (the children would be traced too) and when the budget runs out."""
    import subprocess
    if any(k.startswith(("ROCPROF", "ROCP_TOOL")) for k in os.environ):
        return None
    res, t0 = {}, time.time()
    for w in ("fb15k237_cpg", "wn18rr_cpg", "fb15k237_plain"):
        left = budget_s - (time.time() - t0)
        if left < 25:
            break
        try:
            fed = ["512", "1000", "--with-sampler"] if w == "fb15k237_cpg" else []      # (... and the loop fed by the device samplers, once)
            cp = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_train.py"), w] + fed, capture_output=True, text=True,
                                timeout=min(90.0, left))
            lines = [json.loads(ln) for ln in cp.stdout.splitlines() if ln.startswith("{")]
            if cp.returncode == 0 and lines:
                d = lines[0]
                res[w] = {"ms_per_step": d["ms_per_step"], "B": d["B"], "L": d["L"], "trainable_parameters": d["trainable_parameters"],
                          "floor_ms": d["roofline"]["floor_ms"], "frac_of_floor": d["roofline"]["frac"], "bound": d["roofline"]["bound"]}
                for x in lines[1:]:
                    if "sampler" in x:
                        res[w].setdefault("fed_by_device_sampler_ms_per_step", {})[x["sampler"]] = x["ms_per_step"]
            else:
                res[w] = {"error": (cp.stderr or cp.stdout)[-300:]}
        except Exception as e:      # (a timeout, a missing file: the line goes out without this entry)
            res[w] = {"error": repr(e)[:300]}
    if res:
        res["how"] = ("tools/bench_train.py per workload in a child process: host clock over 20 steps after 3, synthetic batches resident on the "
                      "device; floor = the larger of AMSGrad's slot traffic at 8 TB/s and the step's products at 2.5 PF")
    return res


def pmc_traffic(entry, workload, Q, kernel, exact=None):
    """HBM bytes per launch of `kernel`: NOT measured in this run -- replayed from the committed PMC summary of the
    same command (separate --pmc FETCH_SIZE / WRITE_SIZE passes, gfx950 correction applied); provenance recorded."""
    v, path = _profile_entry("*pmc_traffic*.json", workload, Q, kernel, exact)
    entry["traffic"] = v["hbm_bytes_per_launch"] if v else None
    if v:
        entry["traffic_source"] = "%s (rocprofv3 --pmc passes of this command, committed; not collected in this run)" % path


def pmc_mfma_busy(entry, workload, Q, kernel, exact=None):
    v, path = _profile_entry("*pmc_mfma_busy*.json", workload, Q, kernel, exact)
    if v:
        entry["pmc"] = {"mfma_busy_frac": v["mfma_busy_frac"], "effective_clock_ghz": v["effective_clock_ghz"],
                        "source": "%s (SQ_VALU_MFMA_BUSY_CYCLES, GRBM_GUI_ACTIVE; committed, not collected in this run)" % path}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="fb15k237_cpg")
    ap.add_argument("--mode", choices=["query", "entity"], default="query")
    ap.add_argument("--queries", type=int, default=None)
    ap.add_argument("--order", choices=["shuffled", "sorted"], default="shuffled")
    ap.add_argument("--full", action="store_true",
                    help="also every secondary measurement and check: resident-input and per-pass timings, the fp32-exact comparison, "
                         "the drop-in API timings, per-kernel rooflines, the band audit, the 10M-entity blocks, the training lines, "
                         "the CPU baseline (the --no-* switches below leave parts out)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="CPU-baseline budget per thread setting")
    ap.add_argument("--score-mode", choices=["f32", "bf16x3"], default="bf16x3")
    ap.add_argument("--profile-every", type=int, default=10,
                    help="--full: HIP-event timing of the dominant kernels on every N-th timed step (an event pair around a launch "
                         "costs the stream a few microseconds of pipeline drain; 1 = every step)")
    ap.add_argument("--topk", type=int, default=0,
                    help="entity mode: also select and exchange the per-shard top-k of the filtered rows (SURVEY 8(e) step 3)")
    ap.add_argument("--no-group-next", action="store_true", help="--h2d overlap with every pass sorting its own batch by relation (A/B against coper_group_next)")
    ap.add_argument("--no-post-next", action="store_true", help="--h2d overlap with the ranks copied out by a launch of their own behind every pass (A/B against coper_post_i32_next)")
    ap.add_argument("--h2d", choices=["overlap", "kernel", "sdma"], default="overlap",
                    help="how a pass's pinned int32 batch reaches the device: read over PCIe by extra workgroups of the PREVIOUS pass's "
                         "encoder launch (coper_stage_ids_next), by coper_widen_ids in front of the pass (one launch), or by a "
                         "copy-engine transfer followed by a widening pass")
    ap.add_argument("--launch-timeout", type=int, default=1200,
                    help="self-launched ranks (--gpus N from a plain shell) are stopped after this many seconds")
    ap.add_argument("--no-scale", action="store_true", help="skip the 10M-entity blocks (scale, HBM-regime roofline)")
    ap.add_argument("--no-extras", action="store_true", help="main line only: no f32 comparison, PCIe-inclusive loop, 10M blocks")
    ap.add_argument("--no-train-lines", action="store_true", help="skip the training-step block (three child processes, ~10 s each)")
    ap.add_argument("--scale-side-communicator", action="store_true", help="scale block: the side stream's two collectives on a communicator of their own (EntityShardedRanker(side_communicator=True))")
    ap.add_argument("--no-scale-overlap", action="store_true", help="scale block: steps 1 - 2 of the next chunk on the count launch's own stream (A/B against the side stream)")
    ap.add_argument("--scale-steps", type=int, default=None, help="timed passes of the scale block (default min(steps, 10))")
    ap.add_argument("--per-rank-of", type=int, default=8,
                    help="N = 1 only: also time ONE rank's share of the scale pass at this world size (its entity shard, its "
                         "relations' share of the encoder, no collectives) and print it as scale.projected; 0 = skip")
    ap.add_argument("--dist-backend", default="nccl",
                    help="torch.distributed backend (nccl = RCCL).  gloo + several ranks on one GPU is a debugging aid "
                         "for the multi-process path on a single-GPU box; its numbers mean nothing")
    return ap.parse_args()


def device_params(md, seed, device, shard=None):
    """Random-init weights of the named architecture.  Small tensors come from the seeded numpy generator; an
    entity table too large to build on the host is drawn on the device in independently seeded row blocks
    (coper_amd.data.synthetic_entity_rows_device): the same values whatever the sharding."""
    from coper_amd import data as cdata
    big = int(md["num_ent"]) * int(md["ent_emb_size"]) > (1 << 28)
    p = cdata.synthetic_params(md, seed, skip=("ent_emb", "pred_bias") if big else ())
    if big:
        lo, hi = shard if shard is not None else (0, int(md["num_ent"]))
        p["ent_emb"], p["pred_bias"] = cdata.synthetic_entity_rows_device(md, seed, device, lo, hi)
    return p, big


def cpu_baseline(md, params, q, seconds):
    """SURVEY 8(d) CPU baseline (kind "port": the reference's own CPU path needs TensorFlow 1.14): the reference pass
    restated on torch-CPU fp32 library kernels (conv2d / mm / bmm with the generated dense weights materialised
    [B,F,d] as models.py:70,412) + the literal per-row argsort ranker (metrics.py:44-57), B = 512 as every shipped
    config, on a bounded sample of the same workload: once on all host cores of this process, once on one."""
    import torch
    from oracle.coper_oracle_torch import TorchCPUModel
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    tm = TorchCPUModel(params, md)
    Q, bs = len(q["e1"]), 512

    def run(threads, budget):
        torch.set_num_threads(threads)
        done, t0 = 0, time.perf_counter()
        while done < Q:
            e = min(Q, done + bs)
            ip = q["filt_indptr"][done:e + 1]
            tm.eval_pass(q["e1"][done:e], q["rel"][done:e], q["e2"][done:e], ip - ip[0], q["filt_idx"][ip[0]:ip[-1]], batch_size=bs)
            done = e
            if time.perf_counter() - t0 >= budget:
                break
        dt = time.perf_counter() - t0
        return done / dt, done, dt

    prev = torch.get_num_threads()
    # "all cores": the library threads are given every core this process may run on; oversubscribed thread pools can
    # be slower than fewer threads (a 512-batch bmm on 256 hardware threads), so one batch is timed at a few thread
    # counts first and the budget is spent on the fastest -- `cores` reports the threads actually used
    cand = sorted({c for c in (cores, cores // 2, 64, 32, 16) if 1 < c <= cores}, reverse=True) or [cores]
    calib = {c: run(c, 0.0)[0] for c in cand}
    best = max(calib, key=calib.get)
    v_all, n_all, t_all = run(best, seconds)
    v_one, n_one, t_one = run(1, seconds)
    torch.set_num_threads(prev)
    what = ("torch-CPU fp32 forward (conv2d, mm, bmm over materialised [B,F,d] generated weights), logits for all entities, "
            "dense mask, per-row np.argsort (single-threaded, as the reference's Python loop); batches of %d" % bs)
    return {"value": v_all, "unit": "triples/s", "cores": best, "host_cores": cores, "kind": "port",
            "sample": "%d queries of the same workload (%.1f s): %s" % (n_all, t_all, what),
            "threads_tried": {str(c): round(v, 1) for c, v in calib.items()},
            "one_core": {"value": v_one, "unit": "triples/s", "cores": 1, "sample": "%d queries (%.1f s)" % (n_one, t_one)}}


class Ctx(object):
    pass


def timed_passes(ctx, step, steps):
    """The driver contract: barrier + synchronize, EXACTLY `steps` passes, synchronize + barrier, MAX over ranks."""
    import gc
    import torch
    import torch.distributed as dist
    # the interpreter's cyclic collector stays out of the timed passes (a generation-2 sweep over this process's heap takes tens of
    # milliseconds -- the region is ten): switched off inside, back on after.  Nothing of the measured work changes.  (NOT collected
    # here: a collection between the warm-up passes and the region leaves the device idle for ~100 ms, and the region then runs on
    # its way up from the idle clocks -- measured: 0.552 against 0.483 ms per pass on one box.)
    gc_was_on = gc.isenabled()
    gc.disable()
    if ctx.use_dist:
        dist.barrier()
    torch.cuda.synchronize(ctx.device)
    t0 = time.perf_counter()
    out = None
    trace = [] if os.environ.get("COPER_BENCH_TRACE") else None
    if trace is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    evs = []
    for i in range(steps):
        out = step(i)
        if trace is not None:
            trace.append(time.perf_counter() - t0)
            evs.append(torch.cuda.Event(enable_timing=True))
            evs[-1].record()
    if trace is not None:
        ev1.record()
    torch.cuda.synchronize(ctx.device)
    if ctx.use_dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    if gc_was_on:
        gc.enable()
    if trace is not None:
        print("timed_passes: host issue times (ms) %s, end %.3f, device-side first-to-last %.3f" % (
            " ".join("%.3f" % (t * 1e3) for t in trace[:4]), dt * 1e3, ev0.elapsed_time(ev1)), file=sys.stderr)
        print("   device-side per pass: %s" % " ".join("%.3f" % a.elapsed_time(b) for a, b in zip([ev0] + evs, evs)), file=sys.stderr)
    if ctx.use_dist:
        tmax = torch.tensor([dt], device=ctx.device if ctx.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    return dt, out


def settle(ctx, step, seconds):
    """Untimed passes, back to back, until `seconds` have gone by (checked every 8 passes); returns how many ran.  With a
    process group the ranks stop together: a pass may hold collectives, so every rank must run the same number."""
    import torch
    import torch.distributed as dist
    torch.cuda.synchronize(ctx.device)
    t0, n = time.perf_counter(), 0
    while True:
        for _ in range(8):
            step()
        n += 8
        torch.cuda.synchronize(ctx.device)
        done = time.perf_counter() - t0 >= seconds
        if ctx.use_dist:
            flag = torch.tensor([1 if done else 0], device=ctx.device if ctx.backend == "nccl" else "cpu", dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            done = bool(flag.item())
        if done:
            return n


def dump_outputs(out_dir, arrays, prefix=""):
    """`arrays` (name -> tensor / array with one row per query) as out_dir/<prefix><name>.npy in float64 (every value these
    paths return -- int32 ranks and counts, int64 entity ids, float32 scores -- is exact in it).  Beyond DUMP_LIMIT_BYTES in
    all, the same seeded sample of rows from every array, its row numbers in <prefix>sample_rows.npy."""
    arrays = {k: np.asarray(v.cpu() if hasattr(v, "cpu") else v).astype(np.float64) for k, v in arrays.items() if v is not None}
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        n = len(next(iter(arrays.values())))
        keep = int(DUMP_LIMIT_BYTES // (total / n + 8))       # (+ 8 bytes a row: its number)
        rows = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
        arrays = {k: a[rows] for k, a in arrays.items()}
        arrays["sample_rows"] = rows.astype(np.float64)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, prefix + k + ".npy"), a)


def event_times(ctx, step, steps):
    """Per-pass durations (ms) from HIP events on the launch stream, no host synchronisation between passes."""
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for i in range(steps):
        ev[i][0].record()
        step(i)
        ev[i][1].record()
    torch.cuda.synchronize(ctx.device)
    return [a.elapsed_time(b) for a, b in ev]


def score_kernel_name(mode, d):
    """The count kernel that serves this shape (kernels_score3_bf16.hip serves every d <= 320)."""
    return "k_score_count_f32" if mode == "f32" else "k_score_count3_bf16x3"


def score_roofline(ctx, kname, mode, Q, n_local, d, t_ms, workload, want_pmc=True, exact=None):
    """The score kernel against the lower of its two roofs at this shape.  ALGORITHMIC figures (fused
    rank): flops = 2 Q n d; bytes = the entity table once (fp32 rows or two bf16 planes: 4 B per value) + pred_bias
    + h in + counters out."""
    fl = 2.0 * Q * n_local * d
    by = n_local * d * 4.0 + n_local * 4.0 + Q * d * 4.0 + Q * 8.0
    peak = PEAK_F32_MFMA_TFLOPS if mode == "f32" else PEAK_BF16_MFMA_TFLOPS
    if by / (PEAK_HBM_GBS * 1e9) > fl / (peak * 1e12):
        ach = by / (t_ms * 1e-3) / 1e9
        e = {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": ach / PEAK_HBM_GBS,
             "avg_launch_ms": t_ms, "algorithmic_bytes": by, "algorithmic_tflops": fl / (t_ms * 1e-3) / 1e12}
    else:
        ach = fl / (t_ms * 1e-3) / 1e12
        e = {"bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
             "avg_launch_ms": t_ms, "algorithmic_flops": fl, "algorithmic_gbs": by / (t_ms * 1e-3) / 1e9}
        if mode != "f32":
            e["note"] = "3 hardware 16-bit MFMA products per algorithmic product: hardware MFMA utilisation = 3 x frac"
    e["shape"] = "Q=%d x n=%d x d=%d" % (Q, n_local, d)
    if ctx.world == 1 and want_pmc:
        pmc_traffic(e, workload, Q, "coper::" + kname, exact)
        pmc_mfma_busy(e, workload, Q, "coper::" + kname, exact)
    else:
        e["traffic"] = None
    return e


def run_scale_blocks(ctx, args):
    """BASELINE.json configs[4] on this job's ranks: builds this rank's shard of the 10M-entity model once and runs
    (1) the score kernel's HBM-bound regime (128 queries) and (2) the entity-sharded pass with the top-10 exchange."""
    import torch
    from coper_amd import data as cdata
    from coper_amd.models import ConvE
    from coper_amd.sharding import EntityShardedRanker, shard_bounds
    md = cdata.model_descriptors(SCALE_WORKLOAD)
    d = int(md["ent_emb_size"])
    shard = shard_bounds(md["num_ent"], ctx.world, ctx.rank)
    params, _ = device_params(md, 0, ctx.device, shard)
    # two handles over the same parameter tensors, one per role (coper_config.role): the scorer holds the rank's entity planes and no
    # generated weights, the encoder the generated weights and no planes -- rank_stream runs the encoder's share of chunk n + 1 on a
    # side stream under chunk n's count launch (--no-scale-overlap: one stream, program order)
    model = ConvE(md, device=ctx.device, shard=shard, score_mode="bf16x3", role="score")
    model.load_parameters(params, global_rows=False)
    # (the encoder is split by relation: rank g encodes the queries with rel mod world == g and holds the generated weights of those
    #  relations only -- coper_config.rel_mod_*: 12.8 GB / world)
    enc = ConvE(md, device=ctx.device, shard=shard, score_mode="bf16x3", role="encode", rel_mod=(ctx.world, ctx.rank) if ctx.world > 1 else None)
    enc.load_parameters(params, global_rows=False)
    ranker = EntityShardedRanker(model, encoder=enc, overlap=False if args.no_scale_overlap else None, side_communicator=args.scale_side_communicator)       # (None: from two ranks on; before prepare: the ranks agree on the entity planes' power of two first)
    t0 = time.perf_counter()
    model.prepare()
    enc.prepare()
    torch.cuda.synchronize(ctx.device)
    prepare_ms = (time.perf_counter() - t0) * 1e3
    out = {}

    def make_step(Q, k):
        q = cdata.synthetic_queries(md, Q, seed=0)
        dq = {n: torch.as_tensor(v).to(ctx.device) for n, v in q.items()}
        model.reserve(Q, len(q["filt_idx"]))
        chunk = dict(e1=q["e1"], rel=q["rel"], e2=dq["e2"], filt_indptr=dq["filt_indptr"], filt_idx=dq["filt_idx"])
        return (lambda i=0: ranker.rank(chunk, k=k)), q

    # (1) HBM-bound regime of the score kernel: few queries against a table far larger than the caches
    step, _ = make_step(HBM_REGIME_QUERIES, 0)
    for _ in range(2):
        step()
    model.profile(True)
    model.profile_read("score_count")
    for _ in range(6):
        step()
    torch.cuda.synchronize(ctx.device)
    ms, n = model.profile_read("score_count")
    model.profile(False)
    if n:
        out["hbm_regime"] = score_roofline(ctx, score_kernel_name("bf16x3", d), "bf16x3", HBM_REGIME_QUERIES, model.n_local, d, ms / n,
                                           SCALE_WORKLOAD, exact="coper::k_score_count3_bf16x3<8, 0, 2, 0>")      # (no block maxima)
        out["hbm_regime"]["kernel"] = score_kernel_name("bf16x3", d)
    # (2) the entity-sharded evaluation, top-10 exchanged: a STREAM of distinct chunks (round 6; VERDICT r5 weak 6: rounds 2 - 5
    # re-ranked one chunk, so both host plans of sharding.py were cache hits).  SCALE_CHUNKS different query sets are cycled through
    # EntityShardedRanker.rank_stream: every pass plans its ownership and relation split afresh (one chunk ahead of the device),
    # nothing is read back inside a chunk, the header / audit words are read once per window.
    import itertools
    Q = cdata.CONFIGS[SCALE_WORKLOAD]["queries"]
    qs = [cdata.synthetic_queries(md, Q, seed=s) for s in range(SCALE_CHUNKS)]
    nnz_max = max(len(q["filt_idx"]) for q in qs)

    def chunks_for(qs_):
        out_ = []
        for q in qs_:
            dq = {n: torch.as_tensor(q[n]).to(ctx.device) for n in ("e2", "filt_indptr", "filt_idx")}
            out_.append(dict(e1=q["e1"], rel=q["rel"], e2=q["e2"], e2_dev=dq["e2"], filt_indptr=dq["filt_indptr"], filt_idx=dq["filt_idx"]))
        return out_

    chunks = chunks_for(qs)
    model.reserve(Q, nnz_max)
    enc.reserve(Q, 0)
    first = list(ranker.rank_stream(chunks, k=SCALE_TOPK, window=SCALE_CHUNKS))          # warm-up: every distinct chunk once (and the parity material)
    ranks_all = np.concatenate([r[0].cpu().numpy().astype(np.int32) for r in first])
    top1_id_sum = int(first[0][3][:, 0].sum().item())
    model.profile(True)
    model.profile_read("score_count")
    steps = args.scale_steps or min(args.steps, 12)
    dt, res = timed_passes(ctx, lambda i: list(ranker.rank_stream(itertools.islice(itertools.cycle(chunks), steps), k=SCALE_TOPK,
                                                                   window=SCALE_CHUNKS)), 1)
    ms, n = model.profile_read("score_count")
    model.profile(False)
    again = np.concatenate([r[0].cpu().numpy().astype(np.int32) for r in res[:SCALE_CHUNKS]])
    assert np.array_equal(again, ranks_all[:len(again)]), "the timed stream's ranks differ from the first pass over the same chunks"
    sha = hashlib.sha1(np.ascontiguousarray(ranks_all).tobytes()).hexdigest()
    blk = {"metric": "scored triples/sec (1-vs-all)", "value": Q * steps / dt, "unit": "triples/s", "n_gpus": ctx.world,
           "steps": steps, "ms_per_step": dt / steps * 1e3, "scaling": "strong",
           "config": {"workload": "%s: |E|=%d R2=%d d=%d r=%d, %d DISTINCT chunks of Q=%d queries cycled (the same chunks on every rank; "
                                  "host plans rebuilt for every pass, one chunk ahead)" % (
               SCALE_WORKLOAD, md["num_ent"], md["num_rel"], d, md["rel_emb_size"], SCALE_CHUNKS, Q),
               "parallelism": "entity-sharded x%d (%d rows per rank), top-%d exchanged in one all-gather" % (
                   ctx.world, model.n_local, SCALE_TOPK),
               "score_mode": "bf16x3", "prepare_ms": round(prepare_ms, 2)},
           "mean_rank": float(np.mean(ranks_all)), "mrr": float(np.mean(1.0 / ranks_all)), "ranks_sha1": sha,
           "top1_id_sum": top1_id_sum}
    if n:
        kn = score_kernel_name("bf16x3", d)
        blk["roofline"] = dict(kernel=kn, **score_roofline(ctx, kn, "bf16x3", Q, model.n_local, d, ms / n, SCALE_WORKLOAD,
                                                           want_pmc=ctx.world == 1, exact="coper::k_score_count3_bf16x3<8, 0, 2, 2>"))     # (64-entity block maxima: the top-k launch of a large table)
    exp = SCALE_EXPECTED
    if exp.get("ranks_sha1"):
        # checked by main() AFTER the JSON line is out (every rank must first get through the collectives that follow; the line
        # then still carries the numbers and this flag, and the process exits non-zero)
        blk["ranks_independent_of_world"] = bool(sha == exp["ranks_sha1"])
        if not blk["ranks_independent_of_world"]:
            blk["parity_violation"] = ("entity-sharded ranks at world=%d differ from the single-GPU ranks of the same KG: sha1 %s != %s, "
                                       "mean rank %.6f != %.6f" % (ctx.world, sha, exp["ranks_sha1"], blk["mean_rank"], exp["mean_rank"]))
    blk["config"]["overlap"] = ("steps 1 - 2 of chunk n + 1 on a side stream under chunk n's count launch" if ranker.overlap
                                else "one stream, program order")
    out["scale"] = blk
    model.close()
    enc.close()
    del model, enc, params, ranker
    torch.cuda.empty_cache()
    # What ONE rank of a G-rank job does per chunk, timed on this GPU (a projection, not a measurement of G GPUs): rank 0's shard
    # [0, |E|/G) of the table and EVERYTHING sharding.py runs for it -- the two host plans of every chunk (never cached), the pack /
    # unpack / merge launches, the encoder for the relations rank 0 owns, targets from rows, counts + top-k over the shard, the
    # record -- through the same rank_stream, with every all-gather replaced by a local copy of the rank's own share into all G
    # slots (EntityShardedRanker(emulate_world=...)).  NOT in it: the wire time of the three collectives (<= 9 MB each) and the
    # other ranks' skew.
    G = int(getattr(args, "per_rank_of", 0) or 0)
    if ctx.world == 1 and G > 1:
        shard_g = shard_bounds(md["num_ent"], G, 0)
        params_g, _ = device_params(md, 0, ctx.device, shard_g)
        mg = ConvE(md, device=ctx.device, shard=shard_g, score_mode="bf16x3", role="score")
        mg.load_parameters(params_g, global_rows=False)
        eg = ConvE(md, device=ctx.device, shard=shard_g, score_mode="bf16x3", role="encode", rel_mod=(G, 0))
        eg.load_parameters(params_g, global_rows=False)
        rg = EntityShardedRanker(mg, encoder=eg, emulate_world=(G, 0), overlap=False if args.no_scale_overlap else None)
        mg.prepare()
        eg.prepare()
        mg.reserve(Q, nnz_max)
        eg.reserve(Q, 0)
        chunks_g = chunks_for(qs)
        list(rg.rank_stream(chunks_g, k=SCALE_TOPK, window=SCALE_CHUNKS))
        dtp, _ = timed_passes(ctx, lambda i: list(rg.rank_stream(itertools.islice(itertools.cycle(chunks_g), steps), k=SCALE_TOPK,
                                                                 window=SCALE_CHUNKS)), 1)
        per_rank_ms = dtp / steps * 1e3
        n_enc = int(np.count_nonzero(qs[0]["rel"] % G == 0))
        blk["projected"] = {"world": G, "per_rank_ms": per_rank_ms, "single_gpu_ms": blk["ms_per_step"],
                            "speedup_before_collectives": blk["ms_per_step"] / per_rank_ms,
                            "note": "ONE rank's work of a %d-rank evaluation timed on this GPU through the same rank_stream (shard of %d rows; per "
                                    "chunk: both host plans rebuilt, pack / unpack / merge launches, ~%d of %d queries encoded, targets from rows, "
                                    "counts + top-%d, the record; all-gathers replaced by local copies): a projection -- the wire time of the "
                                    "three collectives (<= 9 MB each, latency-bound) and rank skew are not in it" % (G, mg.n_local, n_enc, Q, SCALE_TOPK)}
        mg.close()
        eg.close()
        del mg, eg, params_g, rg
        torch.cuda.empty_cache()
    return out


def self_launch(args):
    """`python bench.py --gpus N` from a plain shell (no WORLD_SIZE): start the N ranks as fresh child processes of this
    one -- which has not imported torch, let alone touched the GPU, and never exec()s --, one rank per GPU over RCCL
    (`--dist-backend gloo`: ranks may share a GPU; debugging on a one-GPU box).  Rank 0's stdout carries the one JSON
    line and is relayed; a rank that fails takes the others down with it instead of leaving them in the rendezvous."""
    import signal
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    import tempfile
    procs = []
    # rank 0's stdout goes to a temporary FILE, read when the ranks are done (a pipe that nobody drains while this loop polls
    # blocks the rank once the line outgrows the pipe buffer: ADVICE r3)
    out0 = tempfile.TemporaryFile()
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=out0 if r == 0 else sys.stderr, stderr=sys.stderr, start_new_session=True))
    rc, failed = 0, None
    t_start = time.time()
    try:
        live = set(range(args.gpus))
        while live and failed is None:
            time.sleep(0.2)
            if time.time() - t_start > args.launch_timeout:      # a rank stuck in a rendezvous or a collective: bounded, not a hang
                failed, rc = min(live), 124
                print("bench.py: ranks %s still running after %d s" % (sorted(live), args.launch_timeout), file=sys.stderr)
                break
            for r in sorted(live):
                code = procs[r].poll()
                if code is None:
                    continue
                live.discard(r)
                if code != 0:
                    failed, rc = r, code
                    break
    finally:
        if failed is not None:
            print("bench.py: rank %d exited with code %s; stopping the other ranks" % (failed, rc), file=sys.stderr)
        for r, pr in enumerate(procs):
            if pr.poll() is None:                  # our own children, by process group (each is a session leader)
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
    out0.seek(0)
    out = out0.read().decode(errors="replace")
    out0.close()
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    if lines:
        print(lines[-1])
        sys.stdout.flush()
    if failed is None and not lines:
        print("bench.py: rank 0 printed no JSON line", file=sys.stderr)
        rc = 1
    sys.exit(rc if rc else 0)


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)          # never returns
    # stdout carries exactly one line, the JSON result of rank 0: whatever libraries print on the way (RCCL's version
    # banner at communicator creation goes to stdout) is sent to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    from coper_amd import data as cdata
    from coper_amd.models import ConvE
    from coper_amd.sharding import EntityShardedRanker, shard_bounds

    ctx = Ctx()
    ctx.world = world = int(os.environ.get("WORLD_SIZE", "1"))
    ctx.rank = rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        sys.exit("bench.py --gpus %d: WORLD_SIZE is %d (launch with torch.distributed.run --nproc-per-node %d, or from a plain "
                 "shell without WORLD_SIZE: the ranks are then started here)" % (args.gpus, world, args.gpus))
    if args.dist_backend != "nccl":
        local_rank = local_rank % max(1, torch.cuda.device_count())   # debugging: ranks may share a GPU
    torch.cuda.set_device(local_rank)
    ctx.device = device = torch.device("cuda", local_rank)
    ctx.backend = args.dist_backend
    ctx.use_dist = use_dist = world > 1 or bool(os.environ.get("COPER_BENCH_FORCE_DIST"))   # env: the RCCL path with one rank
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(args.dist_backend)

    md = cdata.model_descriptors(args.workload)
    Q = args.queries or cdata.CONFIGS[args.workload]["queries"]
    entity_mode = args.mode == "entity"
    shard = shard_bounds(md["num_ent"], world, rank) if entity_mode else None
    params, big = device_params(md, 0, device, shard)
    model = ConvE(md, device=device, shard=shard, score_mode=args.score_mode)
    model.load_parameters(params, global_rows=not big)
    ranker = EntityShardedRanker(model) if entity_mode else None      # (before prepare: see run_scale_blocks)
    t_prep0 = time.perf_counter()
    model.prepare()
    torch.cuda.synchronize(device)
    prepare_ms = (time.perf_counter() - t_prep0) * 1e3

    # queries: entity mode -> every rank sees the same Q queries; query mode -> Q per rank (weak scaling)
    q = cdata.synthetic_queries(md, Q, seed=0 if entity_mode else rank, order=args.order)
    dev_q = {k: torch.as_tensor(v).to(device) for k, v in q.items()}   # inputs resident in HBM
    nnz = int(len(q["filt_idx"]))
    model.reserve(Q, nnz)
    host_q = dict(q)

    def step(i=0):
        if entity_mode:
            # ids are tiny; the host copies drive the relation split, the device copies feed the kernels
            return ranker.rank(dict(e1=host_q["e1"], rel=host_q["rel"], e2=dev_q["e2"], filt_indptr=dev_q["filt_indptr"],
                                    filt_idx=dev_q["filt_idx"]), k=args.topk)
        # one call per pass, like one session.run of the reference's ranker loop; like ranking_and_hits (and the
        # reference) the pass needs ranks only: tie counts and the embedding itself are not requested
        return model.rank_pass(dev_q["e1"], dev_q["rel"], dev_q["e2"], dev_q["filt_indptr"], dev_q["filt_idx"], filt_nnz=nnz,
                               want_equal=False)

    KERNELS = ("score_count", "dense", "conv", "tail", "band_exact", "group")
    n_passes = [0]            # passes issued before the contract's timed region (reported: the device is warmer than W says)

    def counted(f):
        def g(i=0):
            n_passes[0] += 1
            return f(i)
        return g

    step = counted(step)
    extras = args.full and not args.no_extras
    ranks_np = None                          # (--full: the resident path's ranks, which every other path must reproduce)
    if args.full:
        for _ in range(args.warmup):
            step()
        model.profile(True)
        step()                               # one instrumented untimed pass: fills the library's pool of HIP events
        torch.cuda.synchronize(device)
        for k in KERNELS:
            model.profile_read(k)
        model.profile(False)
        ranks_np = step()[0].cpu().numpy()

    # The SURVEY 8(d) region (the headline in query mode): ids + CSR filters start in pinned host memory, the ranks end in
    # pinned host memory; copies and kernels of a pass are stream-ordered, passes follow each other on the stream.
    pcie_step = None
    pcie_serial = None
    if not entity_mode:
        # One batch as a host would marshal it: [e1 | rel | e2 | filt_indptr | filt_idx] in ONE pinned buffer -> one H2D.
        keys = ("e1", "rel", "e2", "filt_indptr", "filt_idx")
        sizes = [int(np.asarray(q[k]).size) for k in keys]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        # ids and CSR entries travel as int32 (what the reference's placeholders hold; every id of these configs fits) and are
        # widened to the C-ABI's int64 on the device: half the bytes over PCIe for one small elementwise launch
        pin = torch.empty(int(offs[-1]), dtype=torch.int32).pin_memory()
        for k, o, n in zip(keys, offs, sizes):
            assert int(np.max(q[k], initial=0)) < 2 ** 31
            pin[o:o + n].copy_(torch.as_tensor(np.asarray(q[k]).astype(np.int32)))
        stage32 = torch.empty_like(pin, device=device)
        # two staging arrays, used alternately: the pass that runs reads one while the NEXT pass's batch arrives in the other
        stages = [torch.empty(pin.numel(), dtype=torch.int64, device=device) for _ in range(2)]
        views2 = [{k: st[o:o + n] for k, o, n in zip(keys, offs, sizes)} for st in stages]
        cur = [0]
        primed = [False]
        ranks_dev = torch.empty(Q, dtype=torch.int32, device=device)
        out_host = torch.empty(Q, dtype=torch.int32).pin_memory()
        pcie_bytes = pin.numel() * 4 + Q * 4

        def pcie_step(i=0):
            """One pass of the SURVEY 8(d) region: its batch in from pinned host memory, the pass, its ranks out to pinned host
            memory; one stream.  --h2d overlap (default): the batch of pass n + 1 is read over PCIe by extra workgroups of pass
            n's encoder launch (coper_stage_ids_next: they run on CUs the 237 relation tiles leave idle), so every pass still
            moves one batch in and one set of ranks out, but the transfer no longer stands in front of the pass.  --h2d kernel:
            coper_widen_ids in front of the pass (round 3's region); --h2d sdma: a copy-engine transfer and a widening pass.
            (A copy STREAM reached the resident-input rate in tools/pipe_probe.py but stalled for 7 - 30 ms a few times per run
            inside this program: not understood, not used.)"""
            c = cur[0]
            if args.h2d == "overlap":
                if not primed[0]:                          # the very first pass brings its own batch in
                    model.widen_ids(pin, out=stages[c])
                    primed[0] = True
                model.stage_next(pin, stages[1 - c])       # pass n + 1's batch: beside this pass's encoder launch
                if not args.no_group_next:                 # ... where one more workgroup sorts it by relation (coper_group_next)
                    model.group_next(views2[1 - c]["e1"], views2[1 - c]["rel"])
            elif args.h2d == "kernel":
                model.widen_ids(pin, out=stages[c])        # one launch reads the pinned int32 batch over PCIe and writes int64 (coper_widen_ids)
            else:
                stage32.copy_(pin, non_blocking=True)      # copy engine, then a widening pass on the device
                stages[c].copy_(stage32)
            v = views2[c]
            r, _ = model.rank_pass(v["e1"], v["rel"], v["e2"], v["filt_indptr"], v["filt_idx"], filt_nnz=nnz, want_equal=False,
                                   out=ranks_dev)
            if args.h2d == "sdma":
                out_host.copy_(r, non_blocking=True)
            elif args.h2d == "overlap" and not args.no_post_next:
                model.post_next(r, out_host)               # ... and this pass's ranks go out beside the NEXT pass's first launch (coper_post_i32_next)
            else:
                model.copy_out(r, out_host)                # posted writes to the pinned buffer, right behind the last kernel
            if args.h2d == "overlap":
                cur[0] = 1 - c
            return r, None

        pcie_step = counted(pcie_step)
        if args.full:
            for _ in range(max(1, args.warmup)):
                pcie_step()
            model.post_flush()                             # (the last pass's ranks: nothing follows that would carry them out)
            torch.cuda.synchronize(device)
            assert np.array_equal(out_host.numpy(), ranks_np)
        if extras:
            lat = event_times(ctx, pcie_step, args.steps)
            pcie_serial = {"ms_per_pass_median": statistics.median(lat), "ms_per_pass_min": min(lat),
                           "how": "HIP events around H2D + kernels + D2H of each of %d passes (SURVEY 8(d)'s per-pass figure)" % len(lat)}

    # per-pass medians with resident inputs (HIP events, no host synchronisation between passes)
    per_pass = event_times(ctx, step, args.steps) if extras else None

    # the fp32-exact mode on the same queries: its throughput, and where the headline mode's ranks stand against it
    f32_info = None
    if extras and not entity_mode and args.score_mode == "bf16x3" and not big:
        m32 = ConvE(md, device=device, score_mode="f32").load_parameters(params).prepare()
        m32.reserve(Q, nnz)

        def step32(i=0):
            return m32.rank_pass(dev_q["e1"], dev_q["rel"], dev_q["e2"], dev_q["filt_indptr"], dev_q["filt_idx"], filt_nnz=nnz, want_equal=False)

        for _ in range(2):
            step32()
        dt32, res32 = timed_passes(ctx, step32, args.steps)
        r32 = res32[0].cpu().numpy()
        # (1) the fp32 chain's ranker fed the headline mode's own h: the exact band makes these equal for every query
        _, _, hA = model.rank_pass(dev_q["e1"], dev_q["rel"], dev_q["e2"], dev_q["filt_indptr"], dev_q["filt_idx"], filt_nnz=nnz,
                                   want_equal=False, want_h=True)
        r_same = m32.rank(hA, dev_q["e2"], dev_q["filt_indptr"], dev_q["filt_idx"], filt_nnz=nnz, want_equal=False)[0].cpu().numpy()
        # (3) float64 scoring of the same h (torch on the device): what the fp32 chain's own rounding moves
        E64 = model._tensors["ent_emb"].double()
        lg = torch.addmm(model._tensors["pred_bias"].double(), hA.double(), E64.t())
        rows = torch.arange(Q, device=device)
        t64 = lg[rows, dev_q["e2"]].clone()
        row_of = torch.repeat_interleave(rows, dev_q["filt_indptr"][1:] - dev_q["filt_indptr"][:-1])
        lg[row_of, dev_q["filt_idx"]] = -float("inf")
        lg[rows, dev_q["e2"]] = -float("inf")
        r64 = (1 + (lg > t64[:, None]).sum(1)).cpu().numpy()
        del lg, E64

        def agree(a, b):
            d = np.abs(a.astype(np.int64) - b.astype(np.int64))
            return {"fraction_equal": float(np.mean(d == 0)), "max_abs_diff": int(d.max()), "queries": int(len(d))}

        f32_info = {"value": Q * world * args.steps / dt32, "unit": "triples/s", "ms_per_step": dt32 / args.steps * 1e3,
                    "mean_rank": float(np.mean(r32)), "mrr": float(np.mean(1.0 / r32)),
                    "rank_agreement_vs_f32": dict(agree(ranks_np, r_same), note="fp32-chain ranker (COPER_SCORE_F32) fed the headline "
                                                  "mode's own h: comparisons closer than the mode's error are decided by that chain"),
                    "rank_agreement_vs_f32_end_to_end": dict(agree(ranks_np, r32), note="against the fp32-exact mode with its own "
                                                             "encoder: what remains is the two encoders' rounding of h"),
                    "rank_agreement_vs_float64_scoring_of_same_h": agree(ranks_np, r64)}
        m32.close()
        del m32

    # the drop-in entry end to end (host batches in, float64 means out): ranking_and_hits on the loader's dataset object (marshalled
    # once: EvalDataset.staged_for) and on a plain list of 512-query batches (marshalled on every call), host clock
    api = None
    if extras and not entity_mode and not big and args.score_mode == "bf16x3":
        from coper_amd.metrics import ranking_and_hits
        ds = cdata.EvalDataset(q, 512, md["num_ent"])
        batches = list(ds)
        api = {}
        for name_, src in (("eval_dataset", lambda: ds), ("list_of_512_batches", lambda: iter(batches))):
            for _ in range(3):
                out_api = ranking_and_hits(model, None, src(), "bench", return_ranks=True)
            torch.cuda.synchronize(device)
            ts = []
            for _ in range(12):
                t0 = time.perf_counter()
                ranking_and_hits(model, None, src(), "bench")        # (returns host values: the call has waited for its ranks)
                ts.append((time.perf_counter() - t0) * 1e3)
            api[name_] = {"ms_per_call": statistics.median(ts), "ms_per_call_min": min(ts), "ms_per_call_max": max(ts)}
            assert np.array_equal(out_api[3], ranks_np.astype(np.int64))
        api["queries_per_call"] = Q
        api["how"] = "host clock around each of 12 calls (median) of coper_amd.metrics.ranking_and_hits (metrics.py:23-86's signature): PCIe-inclusive, ranks == the pass's"
        if args.workload == "fb15k237_cpg" and Q <= 32768:
            # a set of the REAL test set's size (20,466 triples, both directions: 40,932 queries -- more than one device pass of
            # max_chunk = 32,768): equal chunks staged once, their passes queued back to back, one wait
            q2 = cdata.synthetic_queries(md, 40932, seed=7, order=args.order)
            ds2 = cdata.EvalDataset(q2, 512, md["num_ent"])
            for _ in range(3):
                ranking_and_hits(model, None, ds2, "bench")
            torch.cuda.synchronize(device)
            ts = []
            for _ in range(12):
                t0 = time.perf_counter()
                ranking_and_hits(model, None, ds2, "bench")
                ts.append((time.perf_counter() - t0) * 1e3)
            api["eval_dataset_40932"] = {"ms_per_call": statistics.median(ts), "ms_per_call_min": min(ts), "ms_per_call_max": max(ts),
                                         "triples_per_s": 40932 / (statistics.median(ts) * 1e-3),
                                         "note": "the size of FB15k-237's test set with both directions; two chunks of 20,466"}
            del ds2

    # The driver contract's timed regions come after the secondary measurements above, not before them: the device takes
    # tens of milliseconds of load to leave its idle power state (measured: 0.588 ms per pass over the first 20 passes
    # after setup, 0.549 over 100, 0.532 over 400), and W = 3-5 warm-up passes are 2-3 ms; `pre_timed_passes` says how many
    # passes ran before.  Nothing is carried over but the clocks: barrier + synchronize on both sides, EXACTLY K passes,
    # MAX over ranks.
    resident = None
    if args.full and pcie_step is not None:
        for _ in range(args.warmup):          # the W warm-up passes of this region, right before it
            step()
        dt_res, _ = timed_passes(ctx, step, args.steps)
        resident = {"value": Q * world * args.steps / dt_res, "unit": "triples/s", "ms_per_step": dt_res / args.steps * 1e3,
                    "inputs": "ids + CSR filters resident in HBM before the timed region, ranks left in HBM (round 2's headline)"}
        if per_pass:
            resident["timing"] = {"ms_per_step_median": statistics.median(per_pass), "ms_per_step_min": min(per_pass),
                                  "how": "HIP events on the launch stream around each of %d further passes" % len(per_pass)}
    def profiled_step(i):
        if not os.environ.get("COPER_BENCH_NOPROFILE"):
            model.profile(i % max(1, args.profile_every) == 0)     # per-kernel HIP events on a sample of the timed steps
        return (pcie_step or step)()

    if not args.full:
        settle(ctx, pcie_step or step, SETTLE_S)
    for _ in range(args.warmup):              # the contract's W untimed warm-up steps, right before its K timed ones
        (pcie_step or step)()
    pre_timed = n_passes[0]
    dt, res = timed_passes(ctx, profiled_step if args.full else (pcie_step or step), args.steps)
    model.profile(False)
    # the run-time audit of the exact band over every audited count launch of this process so far (include/coper_hip.h:
    # coper_band_audit; default period: the first launch and every 8th)
    band_audit = None
    if args.full and args.score_mode == "bf16x3":
        ratio, n_pairs = model.band_audit(reset=False)
        band_audit = {"max_error_over_allowance": ratio, "pairs_audited": n_pairs,
                      "note": "largest |logit_x3 - logit_fp32chain| / (tau_q / 2) over the pairs the band walks decided; the mode's ranks are "
                              "the fp32 chain's while this stays below 1 (tests assert <= 0.5 at every operand scale)"}
    if pcie_step is not None:
        model.post_flush()
        torch.cuda.synchronize(device)
        assert model.stale_passes() == 0     # (the guard of coper_group_next: no timed pass ran on a sorting its ids had outlived)
        # what a caller of the timed path holds after its last step: the pass's int32 ranks in pinned host memory
        outputs = {"ranks": out_host.numpy().copy()}
    else:
        outputs = dict(zip(("ranks", "n_equal", "topk_val", "topk_idx"), (t.cpu().numpy() for t in res)))
    if args.full:
        assert np.array_equal(outputs["ranks"], ranks_np)
        assert np.array_equal(res[0].cpu().numpy(), ranks_np)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, outputs, prefix="rank%d_" % rank if world > 1 else "")
    ranks_out = outputs["ranks"]
    kern = {}                                 # (empty in a plain run, which records no kernel events: no roofline block)
    for k in KERNELS:
        ms, n = model.profile_read(k)
        kern[k] = (ms / n) if n else None

    scale = None
    if extras and not args.no_scale and not entity_mode:
        model.close()
        del model, params
        torch.cuda.empty_cache()
        model = None
        scale = run_scale_blocks(ctx, args)

    if rank == 0:
        units = Q * (1 if entity_mode else world) * args.steps
        d = int(md["ent_emb_size"])
        n_local = int(shard[1] - shard[0]) if shard else int(md["num_ent"])
        out = {
            "metric": "scored triples/sec (1-vs-all)", "value": units / dt, "unit": "triples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong" if entity_mode else "weak", "vs_baseline": None,
            "dtype": "f32" if args.score_mode == "f32" else "fp16x3 (fp32 values split into two fp16 terms, 3 fp16 MFMAs per product, fp32 accumulate; "
                     "comparisons closer than the split's error decided by the fp32 chain)",
            "data": "synthetic",
            "config": {"workload": "%s: |E|=%d R2=%d d=%d r=%d, Q=%d queries/pass%s, %s relation order" % (
                args.workload, md["num_ent"], md["num_rel"], d, md["rel_emb_size"], Q,
                "" if entity_mode else " per GPU", args.order),
                "parallelism": ("entity-sharded x%d%s" % (world, ", top-%d exchanged" % args.topk if args.topk else ""))
                if entity_mode else ("query-sharded x%d" % world),
                "score_mode": "f32 (v_mfma_f32_32x32x2_f32, exact)" if args.score_mode == "f32" else
                "bf16x3 = the x3 mode (API name kept): fp16 split since round 3, 3 x v_mfma_f32_16x16x32_f16 (two K = 16 steps each) per "
                "pair of products, ~2^-22 rel.; exact band decided by the fp32 chain", "prepare_ms": round(prepare_ms, 2),
                "inputs": ("SURVEY 8(d) region: every pass brings a batch of ids + CSR filters (int32 in pinned host memory, " + ({"overlap": "the NEXT pass's batch, read over PCIe and widened by extra workgroups of this pass's encoder launch: coper_stage_ids_next" + ("" if args.no_group_next else ", and sorted by relation by one more (coper_group_next: the pass starts with its encoder launch)") + ("" if args.no_post_next else "; the ranks of a pass are posted to pinned host memory by extra blocks of the next pass's first launch: coper_post_i32_next"), "kernel": "read over PCIe and widened by one launch of coper_widen_ids in front of the pass", "sdma": "one copy-engine H2D, widened on the device"}[args.h2d]) + ") in and copies its int32 "
                           "ranks back to pinned host memory (D2H), %d bytes per pass, inside the timed region; one stream"
                           % pcie_bytes) if pcie_step is not None
                else "ids + CSR filters resident in HBM before the timed region",
                "pre_timed_passes": pre_timed,
                "mean_rank": float(np.mean(ranks_out)), "mrr": float(np.mean(1.0 / ranks_out))},
        }
        if resident:
            out["resident_inputs"] = resident
        if pcie_serial:
            out["pcie_per_pass"] = pcie_serial
        if f32_info:
            out["config"]["f32_exact"] = f32_info
        if band_audit:
            out["config"]["band_audit"] = band_audit
        if api:
            out["api"] = api
        if extras and world == 1 and not entity_mode and args.workload == "fb15k237_cpg" and not args.no_train_lines:
            tr = run_train_lines()
            if tr:
                out["train"] = tr
        out["config"]["synthetic_law"] = "ent_emb ~ N(0, 0.1^2) (SURVEY 8(d); rounds 1 - 3: 0.3), pred_bias ~ N(0, 0.1^2)"
        cnt = np.bincount(q["rel"])
        dm = cdata._dims(md)
        F = dm["F"]
        kinfo = {}
        if kern["score_count"]:
            kname = score_kernel_name(args.score_mode, d)
            kinfo[kname] = score_roofline(ctx, kname, args.score_mode, Q, n_local, d, kern["score_count"], args.workload)
        if kern["dense"]:
            fl = 2.0 * Q * F * d                 # ALGORITHMIC flops of the dense launch pair (small + big tiles)
            if args.score_mode == "f32":
                ach = fl / (kern["dense"] * 1e-3) / 1e12
                kinfo["k_dense_big_f32"] = {"bound": "mfma", "achieved": ach, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                                            "frac": ach / PEAK_F32_MFMA_TFLOPS, "avg_launch_ms": kern["dense"]}
                if world == 1:
                    pmc_traffic(kinfo["k_dense_big_f32"], args.workload, Q, "coper::k_dense_big_f32<13>")
            else:
                # ALGORITHMIC bytes ("dense (cached)"): G = DISTINCT relations in the batch (1 for a static layer) --
                # every weight set read ONCE, F*d values in two 16-bit planes -- + the e1 rows in + h out.  The number of
                # <= 128-query tiles (what rounds 1 - 4 multiplied by: 160 for plain ConvE's one static matrix, 33 for WN18RR's 11
                # relations) is the kernel's own re-reading, which the counters show as `traffic`, not algorithmic work.
                # The bound is the larger of bytes / 8 TB/s and flops / 2.5 PF (as score_roofline picks it); the conv runs
                # inside this kernel (x never touches HBM) and counts as flops.
                cc = cnt if md.get("context_rel_out", None) is not None else np.array([Q])
                G = int(np.count_nonzero(cc))
                n_tiles = int(np.sum((cc[cc > 0] + 127) // 128))
                by = G * F * d * 4.0 + Q * d * 4.0 + Q * d * 4.0
                fl_all = fl + 2.0 * Q * F * 9
                ms = kern["dense"]
                t_hbm, t_mfma = by / (PEAK_HBM_GBS * 1e9), fl_all / (PEAK_BF16_MFMA_TFLOPS * 1e12)
                if t_hbm >= t_mfma:
                    ach = by / (ms * 1e-3) / 1e9
                    ki = {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": ach / PEAK_HBM_GBS}
                else:
                    ach = fl_all / (ms * 1e-3) / 1e12
                    ki = {"bound": "mfma", "achieved": ach, "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_BF16_MFMA_TFLOPS}
                ki.update({"avg_launch_ms": ms, "algorithmic_bytes": by, "algorithmic_flops": fl_all, "distinct_weight_sets": G,
                           "query_tiles": n_tiles, "algorithmic_gbs": by / (ms * 1e-3) / 1e9,
                           "algorithmic_tflops": fl_all / (ms * 1e-3) / 1e12})
                kinfo["k_dense_fused_bf16x3"] = ki
                if world == 1:
                    pmc_traffic(kinfo["k_dense_fused_bf16x3"], args.workload, Q, "coper::k_dense_fused_bf16x3")
        if kern["conv"] and args.score_mode == "f32":
            by = Q * (F * 4.0 + d * 4.0)         # ALGORITHMIC bytes: x written + e1 row read
            ach = by / (kern["conv"] * 1e-3) / 1e9
            kinfo["k_conv3x3_bn_relu"] = {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                          "frac": ach / PEAK_HBM_GBS, "avg_launch_ms": kern["conv"]}
            if world == 1:
                pmc_traffic(kinfo["k_conv3x3_bn_relu"], args.workload, Q, "coper::k_conv3x3_bn_relu<4>")
        if kinfo:
            dom = max(kinfo, key=lambda k: kinfo[k]["avg_launch_ms"])   # the dominant kernel of the step
            out["roofline"] = dict(kernel=dom, **kinfo[dom])
            out["roofline"]["all_kernels"] = {k: {kk: vv for kk, vv in v.items() if kk != "note"} for k, v in kinfo.items() if k != dom}
            # share of a pass with resident inputs (its event median; the contract's clock when that was not taken) spent outside
            # the kernels priced above
            pass_ms = resident["timing"]["ms_per_step_median"] if resident and "timing" in resident else (
                resident["ms_per_step"] if resident else dt / args.steps * 1e3)
            out["roofline"]["tail_frac"] = 1.0 - sum(v["avg_launch_ms"] for v in kinfo.values()) / pass_ms
            out["roofline"]["tail_frac_of"] = "resident pass %.4f ms" % pass_ms
            out["roofline"]["other_launches_ms"] = {k: kern[k] for k in ("group", "tail", "band_exact") if kern.get(k)}
        if scale:
            if "hbm_regime" in scale and "roofline" in out:
                out["roofline"]["all_kernels"]["%s@hbm" % scale["hbm_regime"].get("kernel", "k_score_count_bf16x3")] = scale["hbm_regime"]
            out["scale"] = scale["scale"]
        if args.full and not args.no_cpu_baseline and world == 1 and not big:
            host_p = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in cdata.synthetic_params(md, 0).items()}
            out["cpu_baseline"] = cpu_baseline(md, host_p, q, args.cpu_seconds)
            out["config"]["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
        sys.stdout.flush()
        os.dup2(json_fd, 1)
        print(json.dumps(out))
        sys.stdout.flush()
    if use_dist:
        dist.destroy_process_group()
    if scale and scale["scale"].get("parity_violation") and not os.environ.get("COPER_BENCH_NO_ASSERT"):
        sys.exit("PARITY VIOLATION: " + scale["scale"]["parity_violation"])


if __name__ == "__main__":
    main()
