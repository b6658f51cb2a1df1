#!/usr/bin/env python3
"""What the deferred-rows mode of the sampled training step (coper_train_defer_rows) does to the step time as the entity
table grows:

    python tools/bench_train_deferred.py [--shapes fb15k237_cpg,synth1m_cpg,synth10m_cpg] [--reps 20] [--out profiles/train_deferred.json]

Shapes: FB15k-237 CoPER, a 1M-entity table (FB15k-237 CoPER's layers over num_ent = 1,000,000) and `synth10m_cpg`; sampled labels,
B = 512 x L = 1000, ids uniform over the table.  Per shape, one child process with TWO models of the same variables, mode off and mode
on, stepped alternately: 5 warm steps each, then --reps rounds of one `train_step` + a device synchronisation on the host clock per
model -- median [min, max].  Then, on the deferred model, one `train_sync_rows()` (rows up to 5 + reps updates behind), and after 100
further steps one `prepare()` (which syncs first) beside the dense model's `prepare()`.  One JSON document; no threshold is set on these
times (the acceptance property is structural: tests/test_gpu_train_rows.py G.4)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = ["fb15k237_cpg", "synth1m_cpg", "synth10m_cpg"]


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def child(shape, B, L, reps, more_steps):
    import time
    import numpy as np
    import torch
    from coper_amd import data as cdata
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("fb15k237_cpg", num_ent=1_000_000) if shape == "synth1m_cpg" else cdata.model_descriptors(shape)
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.1, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=1e-3)
    E, R, d = md["num_ent"], md["num_rel"], md["ent_emb_size"]
    small = cdata.synthetic_params(md, 0, skip=("ent_emb", "pred_bias"))      # (the tables are drawn on the device: 10 GB at 10M x 256)
    gen = torch.Generator(device="cuda").manual_seed(0)
    ent = torch.randn((E, d), device="cuda", generator=gen) * 0.1
    bias = torch.randn((E,), device="cuda", generator=gen) * 0.1

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    models = {}
    for mode in ("dense", "deferred"):
        p = {k: torch.as_tensor(v) for k, v in small.items()}
        p.update(ent_emb=ent.clone(), pred_bias=bias.clone())
        m = ConvE(md, device="cuda:0").load_parameters(p)
        m.train_init(seed=1, deferred_rows=mode == "deferred")
        models[mode] = m
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(a).cuda()
    bs = [dict(e1=dev(rng.integers(0, E, B)), rel=dev(rng.integers(0, R, B)), lookup_values=dev(rng.integers(0, E, (B, L)).astype(np.int32)),
               e2_multi=dev((rng.random((B, L)) < 0.01).astype(np.float32))) for _ in range(4)]
    for i in range(5):
        for m in models.values():
            m.train_step(bs[i % 4])
    ms = {mode: [] for mode in models}
    for i in range(reps):      # alternating: both modes see the same clocks and the same neighbours
        for mode, m in models.items():
            ms[mode].append(clock(lambda: m.train_step(bs[i % 4])))
    rec = {"shape": shape, "num_ent": E, "d": d, "B": B, "L": L, "device": torch.cuda.get_device_name(0),
           "step_ms": {mode: _stats(v) for mode, v in ms.items()}}
    dm = models["deferred"]
    rec["rows"] = dm.train_row_stats()
    rec["sync_rows_ms"] = clock(dm.train_sync_rows)
    for i in range(more_steps):
        for m in models.values():
            m.train_step(bs[i % 4])
    rec["prepare_ms_after_%d_steps" % more_steps] = {mode: clock(m.prepare) for mode, m in models.items()}
    rec["loss"] = {mode: float(m.last_loss.cpu()[0]) for mode, m in models.items()}
    for m in models.values():
        m.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--lookup", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--more-steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_deferred.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.batch, a.lookup, a.reps, a.more_steps)
    res = []
    for shape in a.shapes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--batch", str(a.batch),
                            "--lookup", str(a.lookup), "--more-steps", str(a.more_steps)], capture_output=True, text=True, timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        rec = json.loads(line[-1]) if r.returncode == 0 and line else {"shape": shape, "failed": r.returncode, "stderr": r.stderr[-400:]}
        res.append(rec)
        print(json.dumps(rec), flush=True)
        if r.returncode not in (0, 1):      # (a child that died of a signal: nothing more is started on the device)
            break
    summary = [{"shape": r["shape"], "deferred_over_dense": r["step_ms"]["deferred"]["median"] / r["step_ms"]["dense"]["median"]}
               for r in res if "step_ms" in r]
    doc = {"tool": "tools/bench_train_deferred.py", "reps": a.reps,
           "clock": "host perf_counter around the call + a device synchronisation; warm (5 steps); one process per shape, the two modes alternating",
           "results": res, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
