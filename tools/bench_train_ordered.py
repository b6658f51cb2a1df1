#!/usr/bin/env python3
"""What ordered rows (coper_train_order_rows) cost per sampled training step:

    python tools/bench_train_ordered.py [--shapes fb15k237_cpg,wn18rr_cpg,synth1m_d64] [--reps 20] [--parent-root DIR]
                                        [--out profiles/train_ordered.json]

Shapes: FB15k-237 and WN18RR CoPER, and `synth1m_d64` (FB15k-237 CoPER's layers over a 1,048,576 x 64 table); sampled labels,
B = 512 x L = 1000, ids uniform over the table.  Configurations, each in a fresh child process:
    default            the default mode
    det                deterministic = 1, where it is served (B * num_ent * 4 <= 512 MiB)
    det_ordered        deterministic = 1 + ordered rows
    deferred           the default mode + deferred rows
    det_ordered_deferred   deterministic = 1 + ordered rows + deferred rows
5 warm steps, then --reps rounds of one `train_step` + a device synchronisation on the host clock: median [min, max].
--parent-root DIR: a checkout of the parent commit with its library built; `default`, `det` and `deferred` are measured on it as well, in
the same run (`parent/...`), to show that they did not move.  For the two ordered configurations a further child runs five steps under
torch.profiler and reports the mean device time of every k_ord_* / k_rows_sumsq_ord launch (`kernels_us`).  One JSON document; no
threshold is set on these times."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.environ.get("COPER_BENCH_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = ["fb15k237_cpg", "wn18rr_cpg", "synth1m_d64"]
CONFIGS = {"default": dict(), "det": dict(deterministic=True), "det_ordered": dict(deterministic=True, ordered_rows=True),
           "deferred": dict(deferred_rows=True), "det_ordered_deferred": dict(deterministic=True, ordered_rows=True, deferred_rows=True)}
ON_PARENT = ("default", "det", "deferred")


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def _md(shape):
    from coper_amd import data as cdata
    if shape == "synth1m_d64":
        md = cdata.model_descriptors("fb15k237_cpg", num_ent=1048576, ent_emb_size=64, emb_h=8, emb_w=8)
    else:
        md = cdata.model_descriptors(shape)
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.1, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=1e-3)
    return md


def child(shape, config, B, L, reps, kernels):
    import time
    import numpy as np
    import torch
    from coper_amd import data as cdata
    from coper_amd.models import ConvE
    md = _md(shape)
    E, R, d = md["num_ent"], md["num_rel"], md["ent_emb_size"]
    rec = {"shape": shape, "config": config, "num_ent": E, "d": d, "B": B, "L": L}
    if config == "det" and B * E * 4 > 512 * 1024 * 1024:
        rec["not_served"] = "deterministic = 1 refuses sampled labels at B * num_ent * 4 > 512 MiB"
        print(json.dumps(rec))
        return
    small = cdata.synthetic_params(md, 0, skip=("ent_emb", "pred_bias"))
    gen = torch.Generator(device="cuda").manual_seed(0)
    p = {k: torch.as_tensor(v) for k, v in small.items()}
    p.update(ent_emb=torch.randn((E, d), device="cuda", generator=gen) * 0.1, pred_bias=torch.randn((E,), device="cuda", generator=gen) * 0.1)
    m = ConvE(md, device="cuda:0").load_parameters(p)
    m.train_init(seed=1, **CONFIGS[config])
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(a).cuda()
    bs = [dict(e1=dev(rng.integers(0, E, B)), rel=dev(rng.integers(0, R, B)), lookup_values=dev(rng.integers(0, E, (B, L)).astype(np.int32)),
               e2_multi=dev((rng.random((B, L)) < 0.01).astype(np.float32))) for _ in range(4)]
    for i in range(5):
        m.train_step(bs[i % 4])
    rec["device"] = torch.cuda.get_device_name(0)
    if kernels:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for i in range(5):
                m.train_step(bs[i % 4])
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            hit = re.search(r"k_ord_\w+|k_rows_sumsq_ord", ev.key)
            if hit:
                dev_us = getattr(ev, "device_time_total", None)
                if dev_us is None:
                    dev_us = ev.cuda_time_total
                name = hit.group(0)
                o = out.setdefault(name, {"launches_per_step": 0.0, "mean_us": 0.0, "us_per_step": 0.0})
                o["launches_per_step"] += ev.count / 5.0
                o["us_per_step"] += dev_us / 5.0
        for o in out.values():
            o["mean_us"] = o["us_per_step"] / o["launches_per_step"]
        rec["kernels_us"] = out
    else:
        ms = []
        for i in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.train_step(bs[i % 4])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec["step_ms"] = _stats(ms)
    rec["loss"] = float(m.last_loss.cpu()[0])
    m.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--lookup", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_ordered.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--config", default="default")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.config, a.batch, a.lookup, a.reps, a.kernels)
    res, stop = [], False
    for shape in a.shapes.split(","):
        runs = [(c, None, False) for c in a.configs.split(",")]
        runs += [(c, a.parent_root, False) for c in a.configs.split(",") if a.parent_root and c in ON_PARENT]
        runs += [(c, None, True) for c in a.configs.split(",") if CONFIGS[c].get("ordered_rows")]
        for config, root, kernels in runs:
            env = dict(os.environ)
            if root:      # the parent commit's package and library, this file's child
                env["COPER_BENCH_ROOT"] = os.path.abspath(root)
                env.pop("COPER_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--config", config, "--reps", str(a.reps), "--batch", str(a.batch),
                   "--lookup", str(a.lookup)] + (["--kernels"] if kernels else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            rec = json.loads(line[-1]) if r.returncode == 0 and line else {"shape": shape, "config": config, "failed": r.returncode,
                                                                          "stderr": r.stderr[-400:]}
            rec["build"] = "parent" if root else "this"
            res.append(rec)
            print(json.dumps(rec), flush=True)
            if r.returncode not in (0, 1):      # (a child that died of a signal: nothing more is started on the device)
                stop = True
                break
        if stop:
            break
    med = {(r["shape"], r["build"], r["config"]): r["step_ms"] for r in res if "step_ms" in r}
    summary = []
    for shape in a.shapes.split(","):
        s = {"shape": shape}
        for num, den in (("det_ordered", "det"), ("det_ordered", "default"), ("det_ordered_deferred", "deferred")):
            if (shape, "this", num) in med and (shape, "this", den) in med:
                s["%s_over_%s" % (num, den)] = med[(shape, "this", num)]["median"] / med[(shape, "this", den)]["median"]
        for c in ON_PARENT:
            if (shape, "this", c) in med and (shape, "parent", c) in med:
                t, p = med[(shape, "this", c)], med[(shape, "parent", c)]
                s["%s_median_inside_parent_range" % c] = bool(p["min"] <= t["median"] <= p["max"])
        summary.append(s)
    doc = {"tool": "tools/bench_train_ordered.py", "reps": a.reps,
           "clock": "host perf_counter around train_step + a device synchronisation; warm (5 steps); one process per configuration",
           "results": res, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
