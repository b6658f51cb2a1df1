#!/usr/bin/env python3
"""What the bit-reproducible training mode (coper_train_config.deterministic) costs, and that the default mode did not move:

    python tools/bench_train_deterministic.py [--lib build/ab/lib_parent.so] [--reps 20] [--out profiles/train_deterministic.json]

Shapes: the three of the training benchmark with sampled labels at B = 512 x L = 1000 (`fb15k237_cpg`, `wn18rr_cpg`,
`fb15k237_plain`) and FB15k-237 1-vs-all from CSR labels (`fb15k237_cpg:csr`, B = 512, the library's chunk width).  Per (library, shape,
mode), each in a child process started fresh: 5 warm steps, then --reps steps, every one `train_step` + a device synchronisation on the
host clock -- median [min, max].  --lib: further libraries measured in the default mode only (the parent commit's build, which has no
other: `git archive` of the parent into a scratch tree, `tools/ab_build.py parent=` there).  The summary holds, per shape, whether this
tree's default-mode median lies within the other library's [min, max], and deterministic / default of this tree.  One JSON document."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = ["fb15k237_cpg", "wn18rr_cpg", "fb15k237_plain", "fb15k237_cpg:csr"]


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def child(shape, deterministic, B, L, reps):
    import ctypes
    import time
    import numpy as np
    import torch
    from coper_amd import _lib, data as cdata
    have = ctypes.CDLL(os.environ.get("COPER_HIP_LIB", _lib.LIB_PATH))
    if not hasattr(have, "coper_train_deterministic"):      # (the parent commit's build: default mode only)
        _lib.PROTOTYPES.pop("coper_train_deterministic", None)
        assert not deterministic
    from coper_amd.models import ConvE
    name, _, labels = shape.partition(":")
    md = cdata.model_descriptors(name)
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.1, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=1e-3)
    E, R = md["num_ent"], md["num_rel"]
    m = ConvE(md, device="cuda:0").load_parameters(cdata.synthetic_params(md, 0))
    m.train_init(seed=1, **({"deterministic": True} if deterministic else {}))
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(a).cuda()

    def batch():
        b = dict(e1=dev(rng.integers(0, E, B)), rel=dev(rng.integers(0, R, B)))
        if labels == "csr":      # four known tails per sample
            rows = [np.unique(r) for r in rng.integers(0, E, (B, 4))]
            b.update(lab_indptr=dev(np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)),
                     lab_idx=dev(np.concatenate(rows).astype(np.int64)))
        else:
            b.update(lookup_values=dev(rng.integers(0, E, (B, L)).astype(np.int32)), e2_multi=dev((rng.random((B, L)) < 0.01).astype(np.float32)))
        return b
    bs = [batch() for _ in range(4)]
    for i in range(5):
        m.train_step(bs[i % 4])
    torch.cuda.synchronize()
    ms = []
    for i in range(reps):
        t0 = time.perf_counter()
        loss = m.train_step(bs[i % 4])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    rec = {"shape": shape, "mode": "deterministic" if deterministic else "default", "B": B, "L": E if labels == "csr" else L,
           "step_ms": _stats(ms), "loss": float(loss.cpu()[0]), "device": torch.cuda.get_device_name(0)}
    m.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--lookup", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_deterministic.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        shape, mode = a.child.rsplit("/", 1)
        return child(shape, mode == "deterministic", a.batch, a.lookup, a.reps)
    res = []
    libs = [""] + [p for p in a.lib.split(",") if p]
    jobs = [(lib, shape, mode) for shape in a.shapes.split(",") for lib in libs for mode in (("default", "deterministic") if not lib else ("default",))]
    for lib, shape, mode in jobs:
        env = dict(os.environ)
        if lib:
            env["COPER_HIP_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%s/%s" % (shape, mode), "--reps", str(a.reps),
                            "--batch", str(a.batch), "--lookup", str(a.lookup)], env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        rec = json.loads(line[-1]) if r.returncode == 0 and line else {"shape": shape, "mode": mode, "failed": r.returncode, "stderr": r.stderr[-400:]}
        rec["library"] = os.path.basename(lib) if lib else "libcoper_hip.so"
        res.append(rec)
        print(json.dumps(rec), flush=True)
        if r.returncode not in (0, 1):      # (a child that died of a signal: nothing more is started on the device)
            break
    summary = []
    for shape in a.shapes.split(","):
        mine = {r["mode"]: r for r in res if r["shape"] == shape and r["library"] == "libcoper_hip.so" and "step_ms" in r}
        row = {"shape": shape}
        if "default" in mine and "deterministic" in mine:
            row["deterministic_over_default"] = mine["deterministic"]["step_ms"]["median"] / mine["default"]["step_ms"]["median"]
        for r in res:
            if r["shape"] == shape and r["library"] != "libcoper_hip.so" and "step_ms" in r and "default" in mine:
                med = mine["default"]["step_ms"]["median"]
                row["default_median_within_" + r["library"]] = bool(r["step_ms"]["min"] <= med <= r["step_ms"]["max"])
                row["default_over_" + r["library"]] = med / r["step_ms"]["median"]
        summary.append(row)
    doc = {"tool": "tools/bench_train_deterministic.py", "reps": a.reps,
           "clock": "host perf_counter around train_step + a device synchronisation; warm (5 steps); a fresh process per row", "results": res,
           "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
