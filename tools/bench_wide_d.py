#!/usr/bin/env python3
"""The count launch and the ranking pass across entity-embedding widths, FB15k-237 CoPER shape (|E| = 14,541, 474 relations,
Q = 20,480), both score modes:

    python tools/bench_wide_d.py [--sizes 256,320,400,512,640] [--modes bf16x3,f32] [--reps 20] [--lib FILE[,FILE]] [--out profiles/wide_d.json]

Up to d = 320 a handle takes the count kernels that hold the whole 128-query tile in LDS, beyond it the ones that hold the tile in
two halves of K (kernels_score3_wide_bf16.hip, k_score_count_wide_f32).  Per (library, d, mode), each in a child process started
fresh (no workspace, clock or cache state carried from one size to the next):
  rank_pass     ConvE.rank_pass, device-synchronised host clock
  score_count   the count launch alone, device events (coper_profile_read), from a second set of passes with the profile on
both warm, median [min, max] over --reps, and the count launch's algorithmic rate 2 Q |E| d / time.  --lib: libraries to compare
(e.g. the parent commit's build beside this tree's); a library that refuses a size is recorded as such.  One JSON document."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = {256: (16, 16), 320: (16, 20), 400: (20, 20), 512: (16, 32), 640: (20, 32)}


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def child(d, mode, reps):
    import time
    import torch
    from coper_amd import _lib, data as cdata
    from coper_amd.models import ConvE
    emb_h, emb_w = SHAPES.get(d, (1, d))
    md = cdata.model_descriptors("fb15k237_cpg", ent_emb_size=d, emb_h=emb_h, emb_w=emb_w)
    Q = 20480
    try:
        m = ConvE(md, device="cuda:0", score_mode=mode).load_parameters(cdata.synthetic_params(md, 0)).prepare()
    except _lib.CoperError as e:
        print(json.dumps({"d": d, "score_mode": mode, "refused": str(e)}))
        return
    q = cdata.synthetic_queries(md, Q, seed=0)
    dq = [torch.as_tensor(q[k]).cuda() for k in ("e1", "rel", "e2", "filt_indptr", "filt_idx")]

    def one():
        m.rank_pass(*dq, want_equal=False)

    for _ in range(3):
        one()
    torch.cuda.synchronize()
    pass_ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one()
        torch.cuda.synchronize()
        pass_ms.append((time.perf_counter() - t0) * 1e3)
    m.profile(True)
    one()
    m.profile_read("score_count")        # (a read returns what accumulated since the last one and starts again)
    count_ms = []
    for _ in range(reps):
        one()
        tot, n = m.profile_read("score_count")
        assert n == 1, n                 # one count launch per pass at this Q
        count_ms.append(tot)
    m.profile(False)
    m.close()
    sc = _stats(count_ms)
    flop = 2.0 * Q * md["num_ent"] * d
    print(json.dumps({"d": d, "score_mode": mode, "Q": Q, "num_ent": md["num_ent"], "rank_pass_ms": _stats(pass_ms), "score_count_ms": sc,
                      "score_count_tflops": flop / (sc["median"] * 1e-3) / 1e12, "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,320,400,512,640")
    ap.add_argument("--modes", default="bf16x3,f32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_d.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        d, mode = a.child.split(":")
        return child(int(d), mode, a.reps)
    res = []
    for lib in (a.lib.split(",") if a.lib else [""]):
        for d in (int(x) for x in a.sizes.split(",")):
            for mode in a.modes.split(","):
                env = dict(os.environ)
                if lib:
                    env["COPER_HIP_LIB"] = os.path.abspath(lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%d:%s" % (d, mode), "--reps", str(a.reps)],
                                   env=env, capture_output=True, text=True, timeout=600)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                rec = json.loads(line[-1]) if r.returncode == 0 and line else {"d": d, "score_mode": mode, "failed": r.returncode, "stderr": r.stderr[-400:]}
                rec["library"] = os.path.basename(lib) if lib else "libcoper_hip.so"
                res.append(rec)
                print(json.dumps(rec), flush=True)
    doc = {"tool": "tools/bench_wide_d.py", "reps": a.reps, "shape": "fb15k237_cpg with ent_emb_size = d, Q = 20480",
           "clock": "rank_pass: host perf_counter around a device-synchronised call; score_count: device events (coper_profile_read); warm",
           "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
