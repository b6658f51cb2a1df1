#!/usr/bin/env python3
"""coper_predict_topk against the other ways to the top-k of (e1, rel, ?), x3 and f32 mode, synthetic models:

    python tools/bench_predict.py [--workloads fb15k237_cpg:512,fb15k237_cpg:20480,wn18rr_cpg:3072] [--k 10] [--reps 20] [--out FILE]
    python tools/bench_predict.py --trace-pass fb15k237_cpg:20480     # five warm predict_topk calls and nothing else (run it under rocprofv3)

Routes, alternating in one process (all see the same minutes of the machine), device-synchronised host clock, warm, median [min, max]
over --reps:
  predict        ConvE.predict_topk(e1, rel, k, CSR)                                    -- exact by the fp32 chain
  dummy_target   encode + target_scores + rank_counts(k) with an invented target        -- the only top-k route before this entry point
                 (the library code on that route is not touched by coper_predict_topk; its answer exempts the invented entity from
                 the filter and, in the x3 mode, is ordered by the mode's own logits)
  rank_pass      ConvE.rank_pass at the same Q                                          -- the scale: same encoder, same score sweep
  score_all_topk encode + score_all + torch.topk (Q <= 2048 only)                       -- the materialising baseline, unfiltered
Also per workload: the share of unresolved queries, chain re-scores per query, the audit ratio (coper_predict_stats) and the bytes the
first predict call added to the ledger after an encode of the same batch.  One JSON document on stdout / in --out."""
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


def _stats(ms):
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def workload(name, Q, k, mode, reps):
    md = cdata.model_descriptors(name)
    lib = _lib.load()
    p = {key: torch.as_tensor(v).cuda() for key, v in cdata.synthetic_params(md, 0).items()}
    q = cdata.synthetic_queries(md, Q, seed=0)
    dq = {key: torch.as_tensor(q[key]).cuda() for key in ("e1", "rel", "e2", "filt_indptr", "filt_idx")}
    m = ConvE(md, device="cuda:0", score_mode=mode).load_parameters(p).prepare()
    h = m.encode(dq["e1"], dq["rel"])
    torch.cuda.synchronize()
    before = lib.coper_live_device_bytes()
    m.predict_topk(None, None, k, dq["filt_indptr"], dq["filt_idx"], h=h)
    torch.cuda.synchronize()
    grew = int(lib.coper_live_device_bytes() - before)
    dummy = torch.zeros_like(dq["e2"])

    def dummy_target():
        hh = m.encode(dq["e1"], dq["rel"])
        return m.rank_counts(hh, m.target_scores(hh, dummy), dummy, dq["filt_indptr"], dq["filt_idx"], k=k)

    routes = {"predict": lambda: m.predict_topk(dq["e1"], dq["rel"], k, dq["filt_indptr"], dq["filt_idx"]),
              "dummy_target": dummy_target,
              "rank_pass": lambda: m.rank_pass(dq["e1"], dq["rel"], dq["e2"], dq["filt_indptr"], dq["filt_idx"], want_equal=False)}
    if Q <= 2048:
        routes["score_all_topk"] = lambda: torch.topk(m.score_all(m.encode(dq["e1"], dq["rel"])), k, dim=1)
    for fn in routes.values():
        for _ in range(3):
            fn()
    m.predict_stats()
    ms = {r: [] for r in routes}
    for _ in range(reps):
        for r, fn in routes.items():
            ms[r].append(_timed(fn))
    st = m.predict_stats()
    m.close()
    nq = max(st["queries"], 1)
    return {"workload": name, "Q": Q, "k": k, "score_mode": mode, "ms": {r: _stats(v) for r, v in ms.items()},
            "unresolved_share": st["unresolved"] / nq, "chain_rescores_per_query": st["rescored"] / nq, "audit_max_ratio": st["max_ratio"],
            "ledger_growth_first_predict_bytes": grew, "row_matrix_bytes": 4 * Q * md["num_ent"]}


def trace_pass(spec, k):
    name, Q = spec.split(":")
    md = cdata.model_descriptors(name)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(cdata.synthetic_params(md, 0)).prepare()
    q = cdata.synthetic_queries(md, int(Q), seed=0)
    dq = [torch.as_tensor(q[key]).cuda() for key in ("e1", "rel", "filt_indptr", "filt_idx")]
    for _ in range(5):
        m.predict_topk(dq[0], dq[1], k, dq[2], dq[3])
    torch.cuda.synchronize()
    m.close()
    print(json.dumps({"traced": "5 predict_topk of %s queries, k = %d, %s, bf16x3" % (Q, k, name)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="fb15k237_cpg:512,fb15k237_cpg:20480,wn18rr_cpg:3072")
    ap.add_argument("--modes", default="bf16x3,f32")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-pass", default=None)
    a = ap.parse_args()
    if a.trace_pass:
        return trace_pass(a.trace_pass, a.k)
    res = []
    for w in a.workloads.split(","):
        name, Q = w.split(":")
        for mode in a.modes.split(","):
            res.append(workload(name, int(Q), a.k, mode, a.reps))
    doc = {"tool": "tools/bench_predict.py", "reps": a.reps, "clock": "host perf_counter around a device-synchronised call, warm",
           "device": torch.cuda.get_device_name(0), "results": res}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
