#!/usr/bin/env python3
"""What the step in three calls costs (coper_train_backward | coper_train_grads_export | coper_train_apply), and that
coper_train_step did not move:

    python tools/bench_train_split.py [--lib build/ab/lib_parent.so] [--reps 20] [--out profiles/train_split.json]
    python tools/bench_train_split.py --kernel-stats DIR      # fold the kernel_stats.csv of a rocprofv3 run of `--child SHAPE/trace` into --out

Shapes: `fb15k237_cpg`, `wn18rr_cpg`, `fb15k237_plain`, sampled labels at B = 512 x L = 1000.  Every row is a child process started
fresh: 5 warm updates, then --reps, each timed on the host clock around the calls + a device synchronisation -- median [min, max].
  step      train_step.  With --lib (the parent commit's build: `git archive` of the parent into a scratch tree, `tools/ab_build.py
            parent=` there) the two libraries ALTERNATE, child by child, --rounds times; the summary says whether this tree's median lies
            within the parent's [min, max] at every shape.
  split     train_backward + train_apply() against step.
  accum/M   M micro-batches (backward + export, accumulating) + train_apply(flat, 1 / M): time per sample at M = 1, 2, 4.
  bits      (with --lib) three deterministic-mode train_steps on seeded inputs, a SHA-256 of the losses, every variable and every
            slot: k_tr_amsgrad gained an argument, and the fused step must still return the parent's bits.
  trace     five warm updates of backward + export + export(accumulate) + apply(flat) and nothing else: run it under
            `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_train_split.py --child SHAPE/trace`, a run
            of its own; --kernel-stats DIR then reads the kernels' average times, computes their bytes from the shapes and the share of
            8 TB/s.  Bytes: export 8 B per element (read g, write flat; accumulate 12), apply-from-flat's k_tr_sumsq 4, k_tr_amsgrad 36
            (g, and m, v, v_hat, p read and written).
`fb15k237_lookup` (--shapes) is the FB15k-237 shape with a looked-up dense layer: a 474 x 4608 x 200 table leaf (bytes are counted
as if every row were present; a batch of 512 holds about two thirds of the relations, so the export's share is an upper bound).
Ranks that share one GPU are a correctness run, not a scaling figure: multi-GPU RCCL training is not measured here."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = ["fb15k237_cpg", "wn18rr_cpg", "fb15k237_plain"]
NEW = ("coper_train_backward", "coper_train_backward_csr", "coper_train_grads_layout", "coper_train_grads_export", "coper_train_apply",
       "coper_train_wmax_carried")


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
    if not hasattr(have, "coper_train_apply"):      # (the parent commit's build: the fused step only)
        for n in NEW:
            _lib.PROTOTYPES.pop(n, None)
        assert mode in ("step", "bits")
    from coper_amd.models import ConvE
    # (`fb15k237_lookup`: the FB15k-237 shape with the dense layer LOOKED UP per relation -- a 474 x 4608 x 200 table, the leaf that
    #  pays the row test in the export and takes the row-count route in the optimizer)
    md = cdata.model_descriptors("fb15k237_cpg", do_parameter_lookup=True) if shape == "fb15k237_lookup" else cdata.model_descriptors(shape)
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.1, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=1e-3)
    E, R = md["num_ent"], md["num_rel"]
    m = ConvE(md, device="cuda:0").load_parameters(cdata.synthetic_params(md, 0))
    m.train_init(seed=1, **({"deterministic": True} if mode == "bits" else {}))
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(a).cuda()
    bs = [dict(e1=dev(rng.integers(0, E, B)), rel=dev(rng.integers(0, R, B)), lookup_values=dev(rng.integers(0, E, (B, L)).astype(np.int32)),
               e2_multi=dev((rng.random((B, L)) < 0.01).astype(np.float32))) for _ in range(4)]
    M = int(mode.split("/")[1]) if mode.startswith("accum/") else 1
    if mode == "bits":      # three deterministic train_steps on seeded inputs: a hash of everything they leave
        import hashlib
        hsh = hashlib.sha256()
        for i in range(3):
            hsh.update(m.train_step(bs[i]).cpu().numpy().tobytes())
        for k in sorted(m._tensors):
            hsh.update(m._tensors[k].cpu().numpy().tobytes())
        slots, powers = m.optimizer_state()
        for k in sorted(slots):
            for part in slots[k]:
                hsh.update(np.ascontiguousarray(part).tobytes())
        print(json.dumps({"shape": shape, "mode": mode, "B": B, "L": L, "sha256": hsh.hexdigest(), "powers": powers}))
        m.close()
        return
    flat = m.train_grads_export() if mode != "step" else None
    state = {"i": 0}

    def update():
        if mode == "step":
            loss = m.train_step(bs[state["i"] % 4])
        elif mode == "split":
            loss = m.train_backward(bs[state["i"] % 4])
            m.train_apply()
        elif mode == "trace":
            loss = m.train_backward(bs[state["i"] % 4])
            m.train_grads_export(flat)
            m.train_grads_export(flat, accumulate=True)
            m.train_apply(flat, 0.5)
        else:
            for k in range(M):
                loss = m.train_backward(bs[(state["i"] + k) % 4])
                m.train_grads_export(flat, accumulate=k > 0)
            m.train_apply(flat, 1.0 / M)
        state["i"] += M
        return loss

    for _ in range(5):
        loss = update()
    torch.cuda.synchronize()
    ms = []
    for _ in range(0 if mode == "trace" else reps):
        t0 = time.perf_counter()
        loss = update()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    layout, total = m.train_grads_layout() if mode != "step" else ({}, 0)
    rec = {"shape": shape, "mode": mode, "B": B, "L": L, "loss": float(loss.cpu()[0]), "device": torch.cuda.get_device_name(0),
           "wmax_carried": m.train_wmax_carried if "coper_train_wmax_carried" in _lib.PROTOTYPES else None,
           "flat_total": total, "trainable_elements": sum(n for _, n in layout.values()), "leaves": len(layout)}
    if ms:
        rec["update_ms"] = _stats(ms)
        rec["us_per_sample"] = 1e3 * rec["update_ms"]["median"] / (M * B)
    m.close()
    print(json.dumps(rec))


def kernel_stats(dirs, doc):
    """rocprofv3 --stats of `--child SHAPE/trace` runs (one directory per shape, named by it) -> doc["kernels"]"""
    out = []
    for d in dirs:
        shape = os.path.basename(os.path.normpath(d))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        rec = next((r for r in doc.get("results", []) if r["shape"] == shape and r.get("flat_total")), None)
        if not files or rec is None:
            out.append({"shape": shape, "absent": "no kernel_stats.csv, or no row of this shape with the vector's length"})
            continue
        n = rec["trainable_elements"]
        per_elem = {"k_tr_grads_export<false>": 8, "k_tr_grads_export<true>": 12, "k_tr_sumsq": 4, "k_tr_amsgrad": 36}
        for r in csv.DictReader(open(files[0])):
            name = r["Name"]
            for key, b in per_elem.items():
                base, _, targ = key.partition("<")
                if base in name and (not targ or "<" + targ in name.replace("(bool)1", "true").replace("(bool)0", "false")):
                    us = float(r["AverageNs"]) / 1e3
                    out.append({"shape": shape, "kernel": key, "calls": int(r["Calls"]), "avg_us": us, "bytes": b * n,
                                "tb_per_s": b * n / us / 1e6, "share_of_8_tb_per_s": b * n / us / 1e6 / 8.0})
    doc["kernels"] = [k for k in doc.get("kernels", []) if k.get("shape") not in {o["shape"] for o in out}] + out
    doc["kernels_note"] = ("bytes from shapes (trainable elements x bytes per element, pads and pointer tables left out); k_tr_sumsq and "
                           "k_tr_amsgrad rows in a trace run are apply-from-flat's only; the project's own stream figures beside them: "
                           "k_tr_amsgrad 0.61, pure stream 0.79 - 0.81 of 8 TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--lookup", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--lib", default="")
    ap.add_argument("--modes", default="split,accum/1,accum/2,accum/4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_split.json"))
    ap.add_argument("--kernel-stats", nargs="*", default=None)
    ap.add_argument("--append", action="store_true", help="add the rows of this run to the document at --out")
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
    res = []
    jobs = []
    for shape in a.shapes.split(","):
        for _ in range(a.rounds):      # the two libraries alternate
            jobs += [(a.lib, shape, "step")] if a.lib else []
            jobs += [("", shape, "step")]
        jobs += [("", shape, mode) for mode in a.modes.split(",") if mode]
        jobs += [(a.lib, shape, "bits"), ("", shape, "bits")] if a.lib else []
    for lib, shape, mode in jobs:
        env = dict(os.environ)
        if lib:
            env["COPER_HIP_LIB"] = os.path.abspath(lib)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%s/%s" % (shape, mode), "--reps", str(a.reps),
                                "--batch", str(a.batch), "--lookup", str(a.lookup)], env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:      # a hung child: its row says so, the rows so far are kept, nothing more is started
            res.append({"shape": shape, "mode": mode, "failed": "timeout", "library": os.path.basename(lib) if lib else "libcoper_hip.so"})
            print(json.dumps(res[-1]), flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        rec = json.loads(line[-1]) if r.returncode == 0 and line else {"shape": shape, "mode": mode, "failed": r.returncode, "stderr": r.stderr[-400:]}
        rec["library"] = os.path.basename(lib) if lib else "libcoper_hip.so"
        res.append(rec)
        print(json.dumps(rec), flush=True)
        if r.returncode not in (0, 1):      # (a child that died of a signal: nothing more is started on the device)
            break
    summary = []
    for shape in a.shapes.split(","):
        import numpy as np
        rows = [r for r in res if r["shape"] == shape and "update_ms" in r]
        mine = [r for r in rows if r["library"] == "libcoper_hip.so"]
        by = lambda mode: [r for r in mine if r["mode"] == mode]
        row = {"shape": shape}
        if by("step"):
            med = float(np.median([r["update_ms"]["median"] for r in by("step")]))
            row["step_ms"] = med
            theirs = [r for r in rows if r["library"] != "libcoper_hip.so"]
            if theirs:
                lo, hi = min(r["update_ms"]["min"] for r in theirs), max(r["update_ms"]["max"] for r in theirs)
                row["parent_step_ms"] = {"min": lo, "median": float(np.median([r["update_ms"]["median"] for r in theirs])), "max": hi}
                row["step_median_within_parent_min_max"] = bool(lo <= med <= hi)
            if by("split"):
                row["split_ms"] = by("split")[0]["update_ms"]["median"]
                row["split_over_step"] = row["split_ms"] / med
        bits = [r["sha256"] for r in res if r["shape"] == shape and r.get("mode") == "bits" and "sha256" in r]
        if len(bits) == 2:
            row["deterministic_step_bits_equal_parent"] = bits[0] == bits[1]
        for r in mine:
            if r["mode"].startswith("accum/"):
                row["us_per_sample_M%s" % r["mode"].split("/")[1]] = r["us_per_sample"]
        summary.append(row)
    doc = {"tool": "tools/bench_train_split.py", "reps": a.reps,
           "clock": "host perf_counter around the calls of one update + a device synchronisation; warm (5 updates); a fresh process per row",
           "not_measured": "multi-GPU RCCL training (ranks sharing one GPU are a correctness run, not a scaling figure)",
           "results": res, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.append and os.path.exists(a.out):
        old = json.load(open(a.out))
        old["results"] += res
        old["summary"] += summary
        doc = old
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
