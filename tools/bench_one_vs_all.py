#!/usr/bin/env python3
"""The 1-vs-all training step (use_negative_sampling = False) INCLUDING the dataset's batch construction, with dense labels
(`OneVsAllTrainDataset`: e2_multi [B, |E|] built on the device per batch -> coper_train_step) and with sparse labels
(`labels="csr"`: three ids per sample -> coper_train_step_csr):

    python tools/bench_one_vs_all.py [--shapes fb15k237_cpg,wn18rr_cpg,e1m_cpg] [--batch 512] [--reps 20] [--lib FILE[,FILE]]
                                     [--out profiles/one_vs_all.json]

Shapes: the two CoPER configurations at B = --batch, and `e1m_cpg`, a table of 1,048,583 entities at d = 12 and B = 129, past the
dense-label call's 512 MiB cap (dense labels are recorded as refused there).  Per (library, shape, labels), each in a child process
started fresh: 5 warm-up steps, then --reps steps, every one `next(batches)` + `train_step` + a device synchronisation on the host
clock -- median [min, max] -- and, from a second set of steps, the same with a synchronisation between the two halves (batch | step).
--lib: libraries to compare (the parent commit's build beside this tree's); a library without the CSR entry points is recorded as
such.  `label_matrix_bytes` is the [B, |E|] float matrix the dense route zero-fills, scatters into and reads once per step and the
CSR route never forms.  One JSON document."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

E1M = dict(num_ent=1048583, num_rel=6, ent_emb_size=12, rel_emb_size=8, emb_h=3, emb_w=4, conv_num_channels=3, conv_filter_height=2,
           conv_filter_width=2, context_rel_conv=None, context_rel_out=[])


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def _samples(num_ent, num_rel, n_rec, tails, seed):
    """n_rec distinct (e1, rel) records with `tails` known tails each, rows ascending"""
    import numpy as np
    rng = np.random.default_rng(seed)
    key = rng.choice(num_ent * num_rel, n_rec, replace=False)
    key.sort()
    rows = [np.unique(r) for r in rng.integers(0, num_ent, (n_rec, tails))]
    return dict(e1=key // num_rel, rel=key % num_rel, tail_indptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                tail_idx=np.concatenate(rows).astype(np.int64))


def child(shape, labels, B, reps):
    import ctypes
    import time
    import torch
    from coper_amd import _lib, data as cdata
    # an older library (--lib: the parent commit's build) has no CSR entry points: bind what it exports
    have = ctypes.CDLL(os.environ.get("COPER_HIP_LIB", _lib.LIB_PATH))
    for name in ("coper_train_step_csr", "coper_train_forward_csr"):
        if not hasattr(have, name):
            _lib.PROTOTYPES.pop(name, None)
    from coper_amd.models import ConvE
    if shape == "e1m_cpg":
        md = dict(cdata._COMMON)
        md.update(E1M)
        B, tails = 129, 5
    else:
        md = cdata.model_descriptors(shape)
        tails = 4
    md.update(use_negative_sampling=False)
    E = md["num_ent"]
    rec = {"shape": shape, "labels": labels, "B": B, "num_ent": E, "d": md["ent_emb_size"], "label_matrix_bytes": B * E * 4}
    if labels == "csr" and "coper_train_step_csr" not in _lib.PROTOTYPES:
        print(json.dumps(dict(rec, absent="the library has no coper_train_step_csr")))
        return
    s = _samples(E, md["num_rel"], 8192, tails, seed=1)
    rec["label_ids_per_batch"] = int(round(B * len(s["tail_idx"]) / 8192.0))
    ds = cdata.OneVsAllTrainDataset(s, E, B, seed=0, device="cuda:0", **({"labels": "csr"} if labels == "csr" else {}))
    m = ConvE(md, device="cuda:0").load_parameters(cdata.synthetic_params(md, 0))
    m.train_init(seed=0)
    it = iter(ds)
    try:
        for _ in range(5):
            m.train_step(next(it))
        torch.cuda.synchronize()
    except _lib.CoperError as e:
        print(json.dumps(dict(rec, refused=str(e))))
        return
    whole, build, step = [], [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.train_step(next(it))
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = next(it)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        m.train_step(b)
        torch.cuda.synchronize()
        build.append((t1 - t0) * 1e3)
        step.append((time.perf_counter() - t1) * 1e3)
    m.close()
    print(json.dumps(dict(rec, batch_and_step_ms=_stats(whole), batch_ms=_stats(build), step_ms=_stats(step),
                          device=torch.cuda.get_device_name(0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="fb15k237_cpg,wn18rr_cpg,e1m_cpg")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "one_vs_all.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        shape, labels = a.child.split(":")
        return child(shape, labels, a.batch, a.reps)
    res = []
    jobs = [(lib, shape, labels) for lib in (a.lib.split(",") if a.lib else [""]) for shape in a.shapes.split(",") for labels in ("dense", "csr")]
    for lib, shape, labels in jobs:
        env = dict(os.environ)
        if lib:
            env["COPER_HIP_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%s:%s" % (shape, labels), "--reps", str(a.reps),
                            "--batch", str(a.batch)], env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        rec = json.loads(line[-1]) if r.returncode == 0 and line else {"shape": shape, "labels": labels, "failed": r.returncode,
                                                                      "stderr": r.stderr[-400:]}
        rec["library"] = os.path.basename(lib) if lib else "libcoper_hip.so"
        res.append(rec)
        print(json.dumps(rec), flush=True)
        if r.returncode not in (0, 1):      # (a child that died of a signal: nothing more is started on the device)
            break
    doc = {"tool": "tools/bench_one_vs_all.py", "reps": a.reps,
           "clock": "host perf_counter around next(batches) + train_step + a device synchronisation; warm (5 steps)", "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
