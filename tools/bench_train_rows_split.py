#!/usr/bin/env python3
"""What the split step of the deferred-rows mode costs (coper_train_rows_backward | _export | _import | _apply), and
that coper_train_step did not move, mode on or off:

    python tools/bench_train_rows_split.py [--lib build/ab/lib_parent.so] [--reps 20] [--out profiles/train_rows_split.json]
    python tools/bench_train_rows_split.py --kernel-stats DIR      # fold the kernel_stats.csv of a rocprofv3 run of `--child SHAPE/trace` into --out

Shapes: `synth1m_cpg` (FB15k-237 CoPER's layers over 1,000,000 entities) and `synth10m_cpg`; sampled labels, B = 512 x L = 1000, ids
uniform over the table.  Every row is a child process started fresh with ONE model (the tables are drawn on the device): 5 warm updates,
then --reps, each timed on the host clock around the calls + a device synchronisation -- median [min, max].
  steps     `train_step` with the mode off, then (the same model, the mode switched on) with the mode on.  With --lib (the parent
            commit's build: `tools/ab_build.py parent=` in a tree of the parent) the two libraries ALTERNATE, child by child; the summary
            says whether this tree's median lies within the parent's [min, max], per mode and shape.
  rows      (this tree's library, the mode on, one child) the fused `train_step`; `train_rows_backward` + `train_rows_apply()`;
            then M = 1, 2, 4 micro-batches of backward + export, M imports, `train_rows_apply(small, 1 / M)`: time per sample; the
            unique rows of a step and the block's bytes (rows x rs x 4 + rows x 4) beside the dense leaf's.
  trace     five warm updates of backward + export + import(first) + apply(small) and nothing else: run it under
            `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_train_rows_split.py --child SHAPE/trace`,
            a run of its own with no counters; --kernel-stats DIR then reads the two kernels' average times and sets them against their
            bytes: export 2 x rows x rs x 4 (read the gradient row, write the block row), import 3 x rows x rs x 4 (read the block row,
            read and write the gradient row; claim, list and catch-up traffic left out), as shares of 8 TB/s.
Ranks that share one GPU are a correctness run, not a scaling figure: multi-GPU training in the mode is not measured here."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = ["synth1m_cpg", "synth10m_cpg"]
NEW = ("coper_train_rows_layout", "coper_train_rows_backward", "coper_train_rows_export", "coper_train_rows_import", "coper_train_rows_apply")


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def child(shape, mode, B, L, reps):
    import ctypes
    import time
    import numpy as np
    import torch
    from coper_amd import _lib, data as cdata
    have = ctypes.CDLL(os.environ.get("COPER_HIP_LIB", _lib.LIB_PATH))
    if not hasattr(have, "coper_train_rows_apply"):      # (the parent commit's build: the fused step only)
        for n in NEW:
            _lib.PROTOTYPES.pop(n, None)
        assert mode == "steps"
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=1_000_000) if shape == "synth1m_cpg" else cdata.model_descriptors(shape)
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.1, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=1e-3)
    E, R, d = md["num_ent"], md["num_rel"], md["ent_emb_size"]
    p = {k: torch.as_tensor(v) for k, v in cdata.synthetic_params(md, 0, skip=("ent_emb", "pred_bias")).items()}
    gen = torch.Generator(device="cuda").manual_seed(0)      # (the tables are drawn on the device: 10 GB at 10M x 256)
    p.update(ent_emb=torch.randn((E, d), device="cuda", generator=gen) * 0.1, pred_bias=torch.randn((E,), device="cuda", generator=gen) * 0.1)
    m = ConvE(md, device="cuda:0").load_parameters(p)
    m.train_init(seed=1, deferred_rows=mode != "steps")
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(a).cuda()
    bs = [dict(e1=dev(rng.integers(0, E, B)), rel=dev(rng.integers(0, R, B)), lookup_values=dev(rng.integers(0, E, (B, L)).astype(np.int32)),
               e2_multi=dev((rng.random((B, L)) < 0.01).astype(np.float32))) for _ in range(4)]
    state = {"i": 0}

    def fused():
        m.train_step(bs[state["i"] % 4])
        state["i"] += 1

    def rows():
        m.train_rows_backward(bs[state["i"] % 4])
        m.train_rows_apply()
        state["i"] += 1

    def accum(M, bufs):
        def update():
            for k in range(M):
                m.train_rows_backward(bs[(state["i"] + k) % 4])
                m.train_rows_export(bufs["small"], accumulate=k > 0, ids=bufs["ids"][k], vals=bufs["vals"][k])
            for k in range(M):
                m.train_rows_import(bufs["ids"][k], bufs["vals"][k], first=k == 0)
            m.train_rows_apply(bufs["small"], 1.0 / M)
            state["i"] += M
        return update

    def timed(fn, n):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return _stats(ms) if ms else None

    rec = {"shape": shape, "mode": mode, "num_ent": E, "d": d, "B": B, "L": L, "device": torch.cuda.get_device_name(0)}
    if mode == "steps":
        rec["step_off_ms"] = timed(fused, reps)
        m.train_defer_rows(True)
        rec["step_on_ms"] = timed(fused, reps)
    else:
        _, total, rs = m.train_rows_layout()
        cap = min(B * (L + 1), E)
        bufs = {"small": torch.zeros(total, device="cuda"), "ids": torch.full((4, cap), -1, device="cuda", dtype=torch.int32),
                "vals": torch.zeros((4, cap, rs), device="cuda")}
        if mode == "trace":
            timed(accum(1, bufs), 0)
        else:
            rec["step_on_ms"] = timed(fused, reps)
            rec["rows_backward_apply_ms"] = timed(rows, reps)
            rec["rows_of_a_batch"] = m.train_row_stats()["rows_last_step"]      # what one export gathers and one import adds
            rec["block_entries"] = cap                                          # (an import is given the whole slot: the rest is padding)
            for M in (1, 2, 4):
                st = timed(accum(M, bufs), reps)
                rec["accum_M%d_ms" % M] = st
                rec["us_per_sample_M%d" % M] = 1e3 * st["median"] / (M * B)
        rows_last = m.train_row_stats()["rows_last_step"]
        per_batch = rec.get("rows_of_a_batch", rows_last)
        rec.update(small_total=total, row_stride=rs, rows_of_the_last_update=rows_last, block_bytes=per_batch * (rs * 4 + 4),
                   dense_leaf_bytes=E * d * 4 + E * 4)
    rec["loss"] = float(m.last_loss.cpu()[0])
    m.close()
    print(json.dumps(rec))


def kernel_stats(dirs, doc):
    """rocprofv3 --stats of `--child SHAPE/trace` runs (one directory per shape, named by it) -> doc["kernels"]"""
    out = []
    for d in dirs:
        shape = os.path.basename(os.path.normpath(d))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        rec = next((r for r in doc.get("results", []) if r["shape"] == shape and r.get("rows_of_a_batch")), None)
        if not files or rec is None:
            out.append({"shape": shape, "absent": "no kernel_stats.csv, or no row of this shape with the rows of a batch"})
            continue
        rows, rs = rec["rows_of_a_batch"], rec["row_stride"]
        per_row = {"k_rows_export": 2 * rs * 4, "k_rows_import": 3 * rs * 4}
        for r in csv.DictReader(open(files[0])):
            for key, b in per_row.items():
                if key in r["Name"]:
                    us = float(r["AverageNs"]) / 1e3
                    out.append({"shape": shape, "kernel": key, "calls": int(r["Calls"]), "avg_us": us, "rows": rows, "bytes": b * rows,
                                "tb_per_s": b * rows / us / 1e6, "share_of_8_tb_per_s": b * rows / us / 1e6 / 8.0})
    doc["kernels"] = [k for k in doc.get("kernels", []) if k.get("shape") not in {o["shape"] for o in out}] + out
    doc["kernels_note"] = ("bytes from shapes (rows of an update x row stride; ids, claim words, list and catch-up traffic left out); the "
                           "project's own stream figures beside them: dense export 0.66 - 0.71, pure stream 0.79 - 0.81 of 8 TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--lookup", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_rows_split.json"))
    ap.add_argument("--kernel-stats", nargs="*", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        shape, mode = a.child.split("/", 1)
        return child(shape, mode, a.batch, a.lookup, a.reps)
    if a.kernel_stats is not None:
        doc = json.load(open(a.out))
        kernel_stats(a.kernel_stats, doc)
        open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc["kernels"]))
        return
    res, jobs = [], []
    for shape in a.shapes.split(","):
        for _ in range(a.rounds):      # the two libraries alternate
            jobs += [(a.lib, shape, "steps")] if a.lib else []
            jobs += [("", shape, "steps")]
        jobs += [("", shape, "rows")]
    for lib, shape, mode in jobs:
        env = dict(os.environ)
        if lib:
            env["COPER_HIP_LIB"] = os.path.abspath(lib)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%s/%s" % (shape, mode), "--reps", str(a.reps),
                                "--batch", str(a.batch), "--lookup", str(a.lookup)], env=env, capture_output=True, text=True, timeout=400)
        except subprocess.TimeoutExpired:      # a hung child: its row says so, the rows so far are kept, nothing more is started
            res.append({"shape": shape, "mode": mode, "failed": "timeout", "library": os.path.basename(lib) if lib else "libcoper_hip.so"})
            print(json.dumps(res[-1]), flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        rec = json.loads(line[-1]) if r.returncode == 0 and line else {"shape": shape, "mode": mode, "failed": r.returncode, "stderr": r.stderr[-400:]}
        rec["library"] = os.path.basename(lib) if lib else "libcoper_hip.so"
        res.append(rec)
        print(json.dumps(rec), flush=True)
        if r.returncode != 0:      # (a child that failed or died of a signal: nothing more is started on the device)
            break
    summary = []
    for shape in a.shapes.split(","):
        import numpy as np
        steps = [r for r in res if r["shape"] == shape and r["mode"] == "steps" and "step_off_ms" in r]
        mine = [r for r in steps if r["library"] == "libcoper_hip.so"]
        theirs = [r for r in steps if r["library"] != "libcoper_hip.so"]
        row = {"shape": shape}
        for key in ("step_off_ms", "step_on_ms"):
            if mine:
                row[key] = float(np.median([r[key]["median"] for r in mine]))
            if mine and theirs:
                lo, hi = min(r[key]["min"] for r in theirs), max(r[key]["max"] for r in theirs)
                row["parent_" + key] = {"min": lo, "median": float(np.median([r[key]["median"] for r in theirs])), "max": hi}
                row[key[:-3] + "_median_within_parent_min_max"] = bool(lo <= row[key] <= hi)
        for r in res:
            if r["shape"] == shape and r["mode"] == "rows" and "rows_backward_apply_ms" in r:
                f = r["step_on_ms"]
                row["rows_backward_apply_ms"] = r["rows_backward_apply_ms"]["median"]
                row["rows_backward_apply_within_fused_min_max"] = bool(f["min"] <= row["rows_backward_apply_ms"] <= f["max"])
                row.update({k: r[k] for k in r if k.startswith("us_per_sample_M") or k in ("rows_of_a_batch", "block_bytes", "dense_leaf_bytes")})
        summary.append(row)
    doc = {"tool": "tools/bench_train_rows_split.py", "reps": a.reps,
           "clock": "host perf_counter around the calls of one update + a device synchronisation; warm (5 updates); a fresh process per row",
           "not_measured": "multi-GPU training in the mode (ranks sharing one GPU are a correctness run, not a scaling figure); the all-gather",
           "results": res, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
