#!/usr/bin/env python3
"""Cached against factored dense layer (coper_config.dense_mode) at inference, x3 mode, synthetic models:

    python tools/bench_factored.py [--workloads fb15k237_cpg,synth10m_cpg] [--reps 20] [--modes cached,factored] [--out FILE]
    python tools/bench_factored.py --trace-pass 2048      # one warm factored pass and nothing else (run it under rocprofv3)

Per workload and per Q: (a) prepare() and (b) rank_pass, device-synchronised host clock, warm, the modes alternating in one process,
min / median / max over --reps; (c) coper_live_device_bytes() after prepare + one pass; (d) prepare + rank_pass ("evaluate after an
update") and the Q where the two modes cross.  --modes cached with COPER_HIP_LIB pointing at another build of the library measures
that build's cached mode with the same loop (the baseline of a change to the library).  One JSON document on stdout / in --out."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from coper_amd import _lib, data as cdata  # noqa: E402
from coper_amd.models import ConvE  # noqa: E402

QS = {"fb15k237_cpg": (512, 2048, 8192, 20480), "synth10m_cpg": (512, 2048, 4096)}


def _stats(ms):
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _fits(md, modes):
    """Device memory the workload needs beside other users: parameters + entity images + the cache (cached mode) + slack."""
    E, d, R = md["num_ent"], md["ent_emb_size"], md["num_rel"]
    F = cdata._dims(md)["F"]
    need = E * d * 4 * 3.2 + md["rel_emb_size"] * F * d * 4 * 2 + (R * F * d * 4 * 2.2 if "cached" in modes else 0) + (8 << 30)
    free, _ = torch.cuda.mem_get_info()
    return need <= free, need, free


def workload(name, modes, reps):
    md = cdata.model_descriptors(name)
    ok, need, free = _fits(md, modes)
    if not ok:
        return {"workload": name, "skipped": "needs ~%.1f GB of device memory, %.1f GB free" % (need / 1e9, free / 1e9)}
    lib = _lib.load()
    p = {k: torch.as_tensor(v).cuda() for k, v in cdata.synthetic_params(md, 0).items()}
    out = {"workload": name, "modes": {}, "lib": os.path.basename(os.environ.get("COPER_HIP_LIB", "in-tree"))}
    models, held = {}, {}
    for mode in modes:
        base = lib.coper_live_device_bytes()
        kw = {} if mode == "cached" else {"dense": mode}        # (a library built before the field existed takes the default)
        models[mode] = ConvE(md, device="cuda:0", score_mode="bf16x3", **kw).load_parameters(p).prepare()
        held[mode] = base
    res = {mode: {"prepare_ms": [], "pass_ms": {}} for mode in modes}
    for Q in QS[name]:
        q = cdata.synthetic_queries(md, Q, seed=0)
        dq = {k: torch.as_tensor(q[k]).cuda() for k in ("e1", "rel", "e2", "filt_indptr", "filt_idx")}
        run = {mode: (lambda m=models[mode]: m.rank_pass(dq["e1"], dq["rel"], dq["e2"], dq["filt_indptr"], dq["filt_idx"], want_equal=False))
               for mode in modes}
        for mode in modes:
            for _ in range(3):
                run[mode]()
            res[mode]["pass_ms"][Q] = []
        for _ in range(reps):
            for mode in modes:                                   # alternating: both modes see the same minutes of the box
                res[mode]["pass_ms"][Q].append(_timed(run[mode]))
    for mode in modes:
        torch.cuda.synchronize()
        res[mode]["live_bytes"] = None
    for _ in range(3):
        for mode in modes:
            models[mode].prepare()
    for _ in range(reps):
        for mode in modes:
            res[mode]["prepare_ms"].append(_timed(models[mode].prepare))
    for mode in modes:
        models[mode].close()
    if True:                                                     # (c) one handle at a time: prepare + one 2,048-query pass
        q = cdata.synthetic_queries(md, 2048, seed=0)
        for mode in modes:
            base = lib.coper_live_device_bytes()
            kw = {} if mode == "cached" else {"dense": mode}
            m = ConvE(md, device="cuda:0", score_mode="bf16x3", **kw).load_parameters(p).prepare()
            m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"], want_equal=False)
            torch.cuda.synchronize()
            res[mode]["live_bytes"] = int(lib.coper_live_device_bytes() - base)
            m.close()
    for mode in modes:
        r = res[mode]
        prep = _stats(r["prepare_ms"])
        o = {"prepare_ms": prep, "rank_pass_ms": {str(Q): _stats(v) for Q, v in r["pass_ms"].items()}, "live_bytes_after_prepare_and_2048_pass": r["live_bytes"]}
        o["prepare_plus_pass_ms_median"] = {str(Q): prep["median"] + float(np.median(v)) for Q, v in r["pass_ms"].items()}
        out["modes"][mode] = o
    if len(modes) > 1:
        a, b = out["modes"]["cached"]["prepare_plus_pass_ms_median"], out["modes"]["factored"]["prepare_plus_pass_ms_median"]
        qs = [Q for Q in QS[name]]
        diff = [b[str(Q)] - a[str(Q)] for Q in qs]               # > 0: cached is ahead
        cross = None
        for i in range(len(qs) - 1):
            if diff[i] < 0 <= diff[i + 1]:
                cross = qs[i] + (qs[i + 1] - qs[i]) * (-diff[i]) / (diff[i + 1] - diff[i])
        out["evaluate_after_update"] = {"factored_minus_cached_ms": {str(Q): v for Q, v in zip(qs, diff)},
                                        "crossover_Q": cross if cross is not None else ("above %d" % qs[-1] if diff[-1] < 0 else "below %d" % qs[0]),
                                        "note": "prepare + rank_pass, medians; linear interpolation between the measured Q"}
    return out


def trace_pass(Q):
    md = cdata.model_descriptors("fb15k237_cpg")
    m = ConvE(md, device="cuda:0", score_mode="bf16x3", dense="factored").load_parameters(cdata.synthetic_params(md, 0)).prepare()
    q = cdata.synthetic_queries(md, Q, seed=0)
    dq = [torch.as_tensor(q[k]).cuda() for k in ("e1", "rel", "e2", "filt_indptr", "filt_idx")]
    for _ in range(5):
        m.rank_pass(*dq, want_equal=False)
    m.prepare()
    torch.cuda.synchronize()
    m.close()
    print(json.dumps({"traced": "5 factored rank_pass of %d queries + 2 prepare, fb15k237_cpg" % Q}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="fb15k237_cpg,synth10m_cpg")
    ap.add_argument("--modes", default="cached,factored")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-pass", type=int, default=0)
    a = ap.parse_args()
    if a.trace_pass:
        return trace_pass(a.trace_pass)
    modes = a.modes.split(",")
    doc = {"tool": "tools/bench_factored.py", "reps": a.reps, "clock": "host perf_counter around a device-synchronised call, warm",
           "device": torch.cuda.get_device_name(0), "results": [workload(w, modes, a.reps) for w in a.workloads.split(",")]}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
