#!/usr/bin/env python3
"""What one rank of an entity-sharded training step costs, phase by phase, on ONE GPU:

    python tools/bench_train_sharded.py [--labels csr|sampled] [--shapes fb15k237_b512,synth1m_b128] [--worlds 1,2,4,8] [--reps 20]
                                        [--parent-root DIR] [--rounds 3] [--out profiles/train_sharded.json]
    python tools/bench_train_sharded.py --labels sampled --deferred [--parent-root DIR] [--rounds 2]

Shapes: FB15k-237 CoPER at B = 512, and its layers over a 1,048,583 x 200 table at B = 128 (or B = 512); ids uniform over the table.
--labels csr (default): sparse 1-vs-all labels, about five positives per row.  --labels sampled: L = 1000 sampled ids per sample,
column 0 positive (coper_train_shard_score_lookup; the whole-table handle of (a) then has ordered rows on, the step a world of one
reproduces); default shapes fb15k237_b512,synth1m_b512, default output profiles/train_sharded_sampled.json.  Each configuration runs
in a fresh child process:
    single             (a) the deterministic whole-table handle, `train_step` on the CSR batch: host clock around the step + a device
                       synchronisation.  With --parent-root DIR (a checkout of the parent commit with its library built) the same on
                       that build, in the same run, the two builds ALTERNATING for --rounds rounds (a process apart, the same code
                       differs by a per cent or two): the path is untouched, so each build's median of medians should lie inside the
                       other's pooled [min, max].
    shard G            (b) rank 0 of G, emulated without the other ranks: a handle that holds rows shard_bounds(E, G, 0), the four
                       calls of a step timed by device events, the exchanges replaced by buffers of the right shape ([B, d] input
                       rows, [G, B, d] shares of dh, G doubles) -- the values mean nothing, the work is the rank's own.  G = 1 is the
                       whole table in the four calls: its score and apply phases are (a)'s scorer and optimizer share.
5 warm steps, then --reps repetitions: median [min, max].  The summary gives, per shape and G, the score and apply phases as a fraction
of G = 1's, the encoder phases, and the projected step of one rank before collectives (the sum of its four phases); with sampled
labels also the score phase split as c + g / G through G = 1 and the largest G (c: what does not divide, the sort over all B (L + 1)
ids and the launches; g: what does, the row gathers and the owned segments).  Multi-GPU scaling
with real RCCL exchanges is NOT measured here.  One JSON document; no threshold is set on these times.
--deferred (with --labels sampled): deferred rows on a shard against the same shard with the mode off.  Configurations:
fb15k237_b512 and synth1m_b512 as rank 0 of 1, synth10m_b512 (10,000,000 x 256) as rank 0 of 8 (1.25M rows); per configuration and
round a process each for this build with the mode off, the parent build (--parent-root) with the mode off, and this build with the mode
on -- the same clock and the same emulated rank as above, and the gather call (which the mode replaces by a kernel of its own) timed
as a fifth phase in front of the four.  The summary pools the rounds (median of the processes' medians, their extremes) and says per
configuration whether the mode-on step lies wholly below the mode-off step, the ratio of the medians, and whether this build's
mode-off median lies inside the parent's [min, max].  Default output profiles/train_sharded_deferred.json.
--forward: the forward-only call (`ConvE.train_shard_forward_only`, sampled labels) of the same emulated rank 0 of G,
over the configurations of --deferred with the mode off and on, a process each: behind the 5 + --reps timed steps of the process, 5
warm forward-only calls, then --reps of them by device events -- once for the loss alone, once with pred_part [B, L] -- beside the
`forward` + `score` phases of the steps of the same process (their sum per step).  The summary says per configuration and mode
whether the forward-only median lies at or below that sum's median, and their ratio.  Default output profiles/train_sharded_forward.json."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.environ.get("COPER_BENCH_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = {"fb15k237_b512": dict(B=512), "synth1m_b128": dict(B=128, num_ent=1048583), "synth1m_b512": dict(B=512, num_ent=1048583),
          "synth10m_b512": dict(B=512, workload="synth10m_cpg")}
DEFERRED_CONFIGS = (("fb15k237_b512", 1), ("synth1m_b512", 1), ("synth10m_b512", 8))      # (shape, G): rank 0 of G is timed
SAMPLED_L = 1000
PHASES = ("forward", "score", "backward", "apply")


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def _md(shape):
    from coper_amd import data as cdata
    over = {k: v for k, v in SHAPES[shape].items() if k not in ("B", "workload")}
    md = cdata.model_descriptors(SHAPES[shape].get("workload", "fb15k237_cpg"), **over)
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.1, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=1e-3)
    return md


def _batches(md, B, labels, n=4):
    import numpy as np
    import torch
    E, R = md["num_ent"], md["num_rel"]
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(a).cuda()
    out = []
    for _ in range(n):
        if labels == "sampled":
            lab = np.zeros((B, SAMPLED_L), np.float32)
            lab[:, 0] = 1.0
            out.append(dict(e1=dev(rng.integers(0, E, B)), rel=dev(rng.integers(0, R, B)),
                            lookup_values=dev(rng.integers(0, E, (B, SAMPLED_L)).astype(np.int32)), e2_multi=dev(lab)))
            continue
        idx = np.sort(rng.integers(0, E, (B, 5)), axis=1)
        idx[:, 1:][idx[:, 1:] == idx[:, :-1]] = E      # (a repeated id: past the table, absent by contract)
        idx = np.sort(idx, axis=1)
        out.append(dict(e1=dev(rng.integers(0, E, B)), rel=dev(rng.integers(0, R, B)), lab_indptr=dev(np.arange(0, 5 * B + 1, 5, dtype=np.int64)),
                        lab_idx=dev(idx.reshape(-1).astype(np.int64))))
    return out


def child(shape, world, reps, labels, deferred=False, gather=False, forward_only=False):
    import time
    import torch
    from coper_amd import data as cdata
    from coper_amd.models import ConvE
    md = _md(shape)
    B, E, d = SHAPES[shape]["B"], md["num_ent"], md["ent_emb_size"]
    rec = {"shape": shape, "num_ent": E, "d": d, "B": B, "world": world, "labels": labels, "deferred_rows": bool(deferred)}
    if labels == "sampled":
        rec["L"] = SAMPLED_L
    if world:
        from coper_amd.sharding import shard_bounds
        lo, hi = shard_bounds(E, world, 0)
    else:
        lo, hi = 0, E
    rec["rows"] = hi - lo
    small = cdata.synthetic_params(md, 0, skip=("ent_emb", "pred_bias"))
    gen = torch.Generator(device="cuda").manual_seed(0)
    p = {k: torch.as_tensor(v) for k, v in small.items()}
    p.update(ent_emb=torch.randn((hi - lo, d), device="cuda", generator=gen) * 0.1, pred_bias=torch.randn((hi - lo,), device="cuda", generator=gen) * 0.1)
    m = ConvE(md, device="cuda:0", shard=(lo, hi)).load_parameters(p, global_rows=False)
    bs = _batches(md, B, labels)
    rec["device"] = torch.cuda.get_device_name(0)
    if not world:
        m.train_init(seed=1, deterministic=True, **(dict(ordered_rows=True) if labels == "sampled" else {}))
        for i in range(5):
            m.train_step(bs[i % 4])
        ms = []
        for i in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.train_step(bs[i % 4])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec["step_ms"] = _stats(ms)
    else:
        m.train_init(seed=1, deterministic=True, entity_sharded=True, **(dict(deferred_rows=True) if deferred else {}))
        rows = torch.randn((B, d), device="cuda", generator=gen) * 0.1
        dh, ls, sq = torch.empty((B, d), device="cuda"), torch.empty(1, device="cuda", dtype=torch.float64), torch.empty(1, device="cuda", dtype=torch.float64)
        dh_all = torch.randn((world, B, d), device="cuda", generator=gen) * 1e-4
        ls_all = torch.ones(world, device="cuda", dtype=torch.float64)
        sq_all = torch.full((world,), 1e-3, device="cuda", dtype=torch.float64)
        times = {k: [] for k in PHASES + ("step",) + (("gather",) if gather else ())}
        for i in range(5 + reps):
            b = bs[i % 4]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            torch.cuda.synchronize()
            if gather:      # (the call in front of the step: in the mode, the rows as of the current update)
                ev[5].record()
                m.train_shard_gather(b["e1"], out=dh)
            ev[0].record()
            m.train_shard_forward(b["e1"], b["rel"], rows)
            ev[1].record()
            (m.train_shard_score_lookup if labels == "sampled" else m.train_shard_score)(b, B, dh, ls)
            ev[2].record()
            m.train_shard_backward(dh_all, ls_all, sq)
            ev[3].record()
            m.train_shard_apply(sq_all)
            ev[4].record()
            torch.cuda.synchronize()
            if i >= 5:
                for j, k in enumerate(PHASES):
                    times[k].append(ev[j].elapsed_time(ev[j + 1]))
                times["step"].append(ev[0].elapsed_time(ev[4]))
                if gather:
                    times["gather"].append(ev[5].elapsed_time(ev[0]))
        rec["phase_ms"] = {k: _stats(v) for k, v in times.items()}
        if forward_only:      # between steps: the loss alone, then with pred_part as well
            rec["forward_plus_score_ms"] = _stats([f + s for f, s in zip(times["forward"], times["score"])])
            for key, want in (("forward_only_ms", False), ("forward_only_pred_ms", True)):
                ms = []
                for i in range(5 + reps):
                    b = bs[i % 4]
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    torch.cuda.synchronize()
                    ev[0].record()
                    m.train_shard_forward_only(b, rows, want)
                    ev[1].record()
                    torch.cuda.synchronize()
                    if i >= 5:
                        ms.append(ev[0].elapsed_time(ev[1]))
                rec[key] = _stats(ms)
        if deferred:
            rec["row_stats_after"] = m.train_row_stats()
    m.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", choices=["csr", "sampled"], default="csr")
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--world", type=int, default=0)
    ap.add_argument("--deferred", action="store_true")
    ap.add_argument("--child-deferred", type=int, default=-1)      # (a child of --deferred: the mode on or off; the gather timed)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--child-forward", action="store_true")       # (a child of --forward: the forward-only calls behind the steps)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.world, a.reps, a.labels, deferred=a.child_deferred == 1, gather=a.child_deferred >= 0, forward_only=a.child_forward)
    if a.forward:
        return main_forward(a)
    if a.deferred:
        return main_deferred(a)
    a.shapes = a.shapes or ("fb15k237_b512,synth1m_b512" if a.labels == "sampled" else "fb15k237_b512,synth1m_b128")
    a.out = a.out or os.path.join(ROOT, "profiles", "train_sharded_sampled.json" if a.labels == "sampled" else "train_sharded.json")
    res, stop = [], False
    for shape in a.shapes.split(","):
        runs = ([(0, None)] + ([(0, a.parent_root)] if a.parent_root else [])) * (a.rounds if a.parent_root else 1)
        runs += [(int(g), None) for g in a.worlds.split(",")]
        for world, root in runs:
            env = dict(os.environ)
            if root:      # the parent commit's package and library, this file's child
                env["COPER_BENCH_ROOT"] = os.path.abspath(root)
                env.pop("COPER_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--world", str(world), "--reps", str(a.reps), "--labels", a.labels]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            rec = json.loads(line[-1]) if r.returncode == 0 and line else {"shape": shape, "world": world, "failed": r.returncode,
                                                                          "stderr": r.stderr[-400:]}
            rec["build"] = "parent" if root else "this"
            res.append(rec)
            print(json.dumps(rec), flush=True)
            if r.returncode not in (0, 1):      # (a child that died of a signal: nothing more is started on the device)
                stop = True
                break
        if stop:
            break
    summary = []
    for shape in a.shapes.split(","):
        s = {"shape": shape}
        single = {}
        for build in ("this", "parent"):      # pooled over the alternating rounds: the median of the processes' medians, their extremes
            rs = [r["step_ms"] for r in res if r["shape"] == shape and "step_ms" in r and r["build"] == build]
            if rs:
                meds = sorted(x["median"] for x in rs)
                single[build] = {"min": min(x["min"] for x in rs), "median": meds[len(meds) // 2], "max": max(x["max"] for x in rs),
                                 "process_medians": [x["median"] for x in rs]}
        if "this" in single:
            s["single_step_ms"] = single["this"]
        if "this" in single and "parent" in single:
            t, p = single["this"], single["parent"]
            s["parent_step_ms"] = p
            s["medians_inside_each_others_range"] = bool(p["min"] <= t["median"] <= p["max"] and t["min"] <= p["median"] <= t["max"])
        ph = {r["world"]: r["phase_ms"] for r in res if r["shape"] == shape and "phase_ms" in r}
        for g in sorted(ph):
            e = {k: ph[g][k]["median"] for k in PHASES}
            e["projected_step_before_collectives_ms"] = sum(e[k] for k in PHASES)
            if 1 in ph:
                e["score_over_world1"] = ph[g]["score"]["median"] / ph[1]["score"]["median"]
                e["apply_over_world1"] = ph[g]["apply"]["median"] / ph[1]["apply"]["median"]
            s["world_%d" % g] = e
        if a.labels == "sampled" and 1 in ph and max(ph) > 1:      # score(G) = c + g / G through G = 1 and the largest G
            gm = max(ph)
            s1, sg = ph[1]["score"]["median"], ph[gm]["score"]["median"]
            per = (s1 - sg) / (1.0 - 1.0 / gm)
            s["score_fit_ms"] = {"through_worlds": [1, gm], "divides_by_world": per, "does_not_divide": s1 - per}
        summary.append(s)
    doc = {"tool": "tools/bench_train_sharded.py", "labels": a.labels, "reps": a.reps,
           "clock": "single: host perf_counter around train_step + a device synchronisation; shard: device events around each of the four calls; "
                    "warm (5 steps); one process per configuration; one GPU, exchanges emulated by buffers (no collective is timed)",
           "results": res, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(summary))


def _pool(rs):
    meds = sorted(x["median"] for x in rs)
    return {"min": min(x["min"] for x in rs), "median": meds[len(meds) // 2], "max": max(x["max"] for x in rs), "process_medians": [x["median"] for x in rs]}


def main_deferred(a):
    if a.labels != "sampled":
        raise SystemExit("--deferred needs --labels sampled (a 1-vs-all step has a gradient in every row)")
    a.out = a.out or os.path.join(ROOT, "profiles", "train_sharded_deferred.json")
    a.rounds = a.rounds if a.rounds != 3 else 2
    configs = [c for c in DEFERRED_CONFIGS if not a.shapes or c[0] in a.shapes.split(",")]
    res, stop = [], False
    for shape, world in configs:
        modes = [("this", 0, None)] + ([("parent", 0, a.parent_root)] if a.parent_root else []) + [("this", 1, None)]
        for build, on, root in modes * a.rounds:
            env = dict(os.environ)
            if root:      # the parent commit's package and library, this file's child
                env["COPER_BENCH_ROOT"] = os.path.abspath(root)
                env.pop("COPER_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--world", str(world), "--reps", str(a.reps), "--labels", "sampled",
                   "--child-deferred", str(on)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            rec = json.loads(line[-1]) if r.returncode == 0 and line else {"shape": shape, "world": world, "deferred_rows": bool(on), "failed": r.returncode,
                                                                          "stderr": r.stderr[-400:]}
            rec["build"] = build
            res.append(rec)
            print(json.dumps(rec), flush=True)
            if r.returncode not in (0, 1):      # (a child that died of a signal: nothing more is started on the device)
                stop = True
                break
        if stop:
            break
    summary = []
    for shape, world in configs:
        s = {"shape": shape, "world": world}
        for key, build, on in (("mode_off", "this", False), ("parent_mode_off", "parent", False), ("mode_on", "this", True)):
            rs = [r["phase_ms"] for r in res if r["shape"] == shape and "phase_ms" in r and r["build"] == build and r["deferred_rows"] == on]
            if rs:
                s[key] = {k: _pool([x[k] for x in rs]) for k in rs[0]}
                s["rows"] = [r["rows"] for r in res if r["shape"] == shape and "rows" in r][0]
        if "mode_on" in s and "mode_off" in s:
            on, off = s["mode_on"]["step"], s["mode_off"]["step"]
            s["mode_on_wholly_below_mode_off"] = bool(on["max"] < off["min"])
            s["mode_off_over_mode_on"] = off["median"] / on["median"]
            s["rows_listed_last_step"] = [r["row_stats_after"]["rows_last_step"] for r in res if r["shape"] == shape and "row_stats_after" in r][0]
        if "mode_off" in s and "parent_mode_off" in s:
            t, p = s["mode_off"]["step"], s["parent_mode_off"]["step"]
            s["mode_off_median_inside_parents_range"] = bool(p["min"] <= t["median"] <= p["max"])
        summary.append(s)
    doc = {"tool": "tools/bench_train_sharded.py --labels sampled --deferred", "reps": a.reps, "rounds": a.rounds, "L": SAMPLED_L,
           "clock": "device events around the gather and each of the four calls of rank 0 of G; step = the four calls; warm (5 steps); one process "
                    "per configuration, mode and round; one GPU, exchanges emulated by buffers (no collective is timed)",
           "results": res, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(summary))


def main_forward(a):
    a.out = a.out or os.path.join(ROOT, "profiles", "train_sharded_forward.json")
    configs = [c for c in DEFERRED_CONFIGS if not a.shapes or c[0] in a.shapes.split(",")]
    res, stop = [], False
    for shape, world in configs:
        for on in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--world", str(world), "--reps", str(a.reps), "--labels", "sampled",
                   "--child-deferred", str(on), "--child-forward"]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            rec = json.loads(line[-1]) if r.returncode == 0 and line else {"shape": shape, "world": world, "deferred_rows": bool(on), "failed": r.returncode,
                                                                          "stderr": r.stderr[-400:]}
            res.append(rec)
            print(json.dumps(rec), flush=True)
            if r.returncode not in (0, 1):      # (a child that died of a signal: nothing more is started on the device)
                stop = True
                break
        if stop:
            break
    summary = []
    for r in res:
        if "forward_only_ms" not in r:
            continue
        fo, fs = r["forward_only_ms"], r["forward_plus_score_ms"]
        s = {"shape": r["shape"], "world": r["world"], "rows": r["rows"], "deferred_rows": r["deferred_rows"], "forward_only_ms": fo,
             "forward_only_pred_ms": r["forward_only_pred_ms"], "step_forward_plus_score_ms": fs,
             "step_forward_ms": r["phase_ms"]["forward"], "step_score_ms": r["phase_ms"]["score"],
             "forward_only_over_forward_plus_score": fo["median"] / fs["median"],
             "forward_only_median_at_or_below_forward_plus_score": bool(fo["median"] <= fs["median"])}
        if "row_stats_after" in r:
            s["row_stats"] = r["row_stats_after"]
        summary.append(s)
    doc = {"tool": "tools/bench_train_sharded.py --forward", "reps": a.reps, "L": SAMPLED_L,
           "clock": "device events around one forward-only call (ConvE.train_shard_forward_only) of rank 0 of G, warm (5 calls) behind the timed steps "
                    "of the same process; beside it the steps' forward + score phases, summed per step; one process per configuration and mode; one "
                    "GPU, exchanges emulated by buffers (no collective is timed)",
           "results": res, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
