#!/usr/bin/env python3
"""What the resident known-facts index costs and saves: predict_topk and rank_pass by three routes, FB15k-237 shapes, bf16x3:

    python tools/bench_known.py [--sizes 512,20480] [--k 10] [--reps 20] [--out FILE]
    python tools/bench_known.py --trace-pass 512        # five warm predict_topk_known calls and nothing else (run it under rocprofv3)

Routes, alternating in one process (all see the same minutes of the machine), device-synchronised host clock, warm, median [min, max]
over --reps:
  (a) device_csr   the explicit-CSR call with a CSR of the same content already on the device   -- the floor: the code before the index
  (b) known        predict_topk_known / rank_pass_known: the filter looked up in the resident index
  (c) host_csr     what a caller without the index does: the batch's CSR assembled in NumPy from the HOST index (a searchsorted over
                   the keys, a gather of the rows), then the explicit-CSR call from host arrays (stage_csr / stage_batch)
The index is the synthetic query set's (`data.known_facts_from_queries`), the batch its first B queries.  (b) - (a) is the cost of the
lookup: three launches, one 8-byte readback, one stream synchronisation.  One JSON document on stdout / in --out."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from coper_amd import data as cdata  # noqa: E402
from coper_amd.models import ConvE  # noqa: E402

NAME = "fb15k237_cpg"


def _stats(ms):
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host_csr(kf, key, num_rel, e1, rel):
    """The batch's CSR from the host index, vectorised NumPy: what `kg_loader.encoded_split` replays per query in Python."""
    qk = e1 * num_rel + rel
    pos = np.minimum(np.searchsorted(key, qk), len(key) - 1)
    found = key[pos] == qk
    start = kf["tail_indptr"][pos]
    n = np.where(found, kf["tail_indptr"][pos + 1] - start, 0)
    ip = np.zeros(len(e1) + 1, np.int64)
    np.cumsum(n, out=ip[1:])
    ix = kf["tail_idx"][np.repeat(start - ip[:-1], n) + np.arange(ip[-1])]
    return ip, ix


def _setup(Q):
    md = cdata.model_descriptors(NAME)
    p = {key: torch.as_tensor(v).cuda() for key, v in cdata.synthetic_params(md, 0).items()}
    q = cdata.synthetic_queries(md, Q, seed=0)
    kf = cdata.known_facts_from_queries(q)
    m = ConvE(md, device="cuda:0", score_mode="bf16x3").load_parameters(p).prepare().set_known_facts(**kf)
    return md, q, kf, m


def workload(md, q, kf, m, B, k, reps):
    R = int(md["num_rel"])
    key = kf["e1"] * R + kf["rel"]
    e1, rel, e2 = (np.ascontiguousarray(q[n][:B]) for n in ("e1", "rel", "e2"))
    ip, ix = host_csr(kf, key, R, e1, rel)
    d = {n: torch.as_tensor(v).cuda() for n, v in (("e1", e1), ("rel", rel), ("e2", e2), ("ip", ip), ("ix", ix))}
    gip, gix = m.known_filter(d["e1"], d["rel"])
    assert torch.equal(gip, d["ip"]) and torch.equal(gix, d["ix"])

    def predict_host():
        hip, hix = host_csr(kf, key, R, e1, rel)
        return m.predict_topk(e1, rel, k, hip, hix)

    def rank_host():
        hip, hix = host_csr(kf, key, R, e1, rel)
        st = m.stage_csr(e2, hip, hix)
        if st is None:
            return m.rank_pass(e1, rel, e2, hip, hix, want_equal=False)
        a, b = m.stage_batch(e1, rel)
        return m.rank_pass(a, b, st[0], st[1], st[2], want_equal=False)

    routes = {
        "predict": {"device_csr": lambda: m.predict_topk(d["e1"], d["rel"], k, d["ip"], d["ix"]),
                    "known": lambda: m.predict_topk_known(d["e1"], d["rel"], k),
                    "host_csr": predict_host},
        "rank_pass": {"device_csr": lambda: m.rank_pass(d["e1"], d["rel"], d["e2"], d["ip"], d["ix"], want_equal=False),
                      "known": lambda: m.rank_pass_known(d["e1"], d["rel"], d["e2"], want_equal=False),
                      "host_csr": rank_host}}
    out = {"B": B, "k": k, "filter_nnz": int(ip[-1]), "index_rows": int(len(key)), "index_nnz": int(kf["tail_idx"].size), "ms": {}}
    for call, rs in routes.items():
        for fn in rs.values():
            for _ in range(3):
                fn()
        ms = {r: [] for r in rs}
        for _ in range(reps):
            for r, fn in rs.items():
                ms[r].append(_timed(fn))
        st = {r: _stats(v) for r, v in ms.items()}
        st["lookup_cost_ms"] = st["known"]["median"] - st["device_csr"]["median"]
        out["ms"][call] = st
    return out


def trace_pass(B, k):
    md, q, kf, m = _setup(B)
    e1, rel = torch.as_tensor(q["e1"]).cuda(), torch.as_tensor(q["rel"]).cuda()
    for _ in range(5):
        m.predict_topk_known(e1, rel, k)
    torch.cuda.synchronize()
    m.close()
    print(json.dumps({"traced": "5 predict_topk_known of %d queries, k = %d, %s, bf16x3" % (B, k, NAME)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,20480")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-pass", type=int, default=None)
    a = ap.parse_args()
    if a.trace_pass:
        return trace_pass(a.trace_pass, a.k)
    sizes = [int(s) for s in a.sizes.split(",")]
    md, q, kf, m = _setup(max(sizes))
    res = [workload(md, q, kf, m, B, a.k, a.reps) for B in sizes]
    m.close()
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                         stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    doc = {"tool": "tools/bench_known.py", "workload": NAME, "score_mode": "bf16x3", "reps": a.reps,
           "clock": "host perf_counter around a device-synchronised call, warm", "device": torch.cuda.get_device_name(0), "commit": commit,
           "results": res}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
