#!/usr/bin/env python3
"""What the backward in phases costs (coper_train_sync_begin | coper_train_sync_next), and that the unchanged routes
did not move:

    python tools/bench_train_sync.py [--lib build/ab/lib_parent.so] [--reps 20] [--rounds 2] [--out profiles/train_sync_bn.json]

Shape: `fb15k237_cpg`, sampled labels, B = 512 x L = 1000, default and deterministic mode.  Every row is a child process started
fresh: 5 warm calls, then --reps, each timed on the host clock around the calls + a device synchronisation -- median [min, max].
  step       train_step.            With --lib (the parent commit's build: `git archive` of the parent into a scratch tree, built there)
  backward   train_backward.        the two libraries ALTERNATE, child by child, --rounds times; the summary says whether this tree's
                                    median lies within the parent's [min, max].
  sync1      the synchronised backward at a world of one: begin + four next, each handed its own part (a view, no copy) -- against
             `backward` this is the cost of cutting the step into five calls (four folds, five small copies, the side streams joined
             at every cut) plus the split FCBN backward.
  rank8      G = 8 handles in one process, B = 64 each, B_global = 512: per phase the other seven ranks' calls run untimed, then rank
             0's call is timed; the row is the sum of rank 0's five calls.  The gather is torch.stack and is not timed.
  bits       (with --lib) deterministic mode: two train_steps and a train_backward on seeded inputs, a SHA-256 of the losses, the flat
             gradient, every variable and every slot -- the kernels that draw dropout masks gained an index offset, and the
             unchanged routes must still return the parent's bits.
Not measured: the four all-gathers of a few hundred bytes over real RCCL, which a data-parallel run adds per micro-batch."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPE = "fb15k237_cpg"
NEW = ("coper_train_sync_begin", "coper_train_sync_begin_csr", "coper_train_sync_next", "coper_train_sync_phase", "coper_train_sync_part_len")


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "n": int(len(a))}


def child(mode, det, B, L, reps):
    import ctypes
    import time
    import numpy as np
    import torch
    from coper_amd import _lib, data as cdata
    have = ctypes.CDLL(os.environ.get("COPER_HIP_LIB", _lib.LIB_PATH))
    if not hasattr(have, "coper_train_sync_begin"):      # (the parent commit's build)
        for n in NEW:
            _lib.PROTOTYPES.pop(n, None)
        assert mode in ("step", "backward", "bits")
    from coper_amd.models import ConvE
    md = cdata.model_descriptors(SHAPE)
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.1, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=1e-3)
    E, R = md["num_ent"], md["num_rel"]
    G = 8 if mode == "rank8" else 1
    Bl = B // G
    p0 = cdata.synthetic_params(md, 0)
    ms_ = [ConvE(md, device="cuda:0").load_parameters(p0) for _ in range(G)]
    for m in ms_:
        m.train_init(seed=1, deterministic=bool(det))
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(a).cuda()
    bs = [dict(e1=dev(rng.integers(0, E, B)), rel=dev(rng.integers(0, R, B)), lookup_values=dev(rng.integers(0, E, (B, L)).astype(np.int32)),
               e2_multi=dev((rng.random((B, L)) < 0.01).astype(np.float32))) for _ in range(4)]
    shard = lambda b, r: {k: v[r * Bl:(r + 1) * Bl] for k, v in b.items()}
    state = {"i": 0}
    if mode == "bits":
        import hashlib
        m, hsh = ms_[0], hashlib.sha256()
        for i in range(2):
            hsh.update(m.train_step(bs[i]).cpu().numpy().tobytes())
        hsh.update(m.train_backward(bs[2]).cpu().numpy().tobytes())
        hsh.update(m.train_grads_export().cpu().numpy().tobytes())
        for k in sorted(m._tensors):
            hsh.update(m._tensors[k].cpu().numpy().tobytes())
        slots, powers = m.optimizer_state()
        for k in sorted(slots):
            for part in slots[k]:
                hsh.update(np.ascontiguousarray(part).tobytes())
        print(json.dumps({"shape": SHAPE, "mode": mode, "deterministic": int(det), "B": B, "L": L, "sha256": hsh.hexdigest()}))
        m.close()
        return

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def call():
        """-> milliseconds of what the mode times"""
        b = bs[state["i"] % 4]
        state["i"] += 1
        m = ms_[0]
        if mode == "step":
            return timed(lambda: m.train_step(b))[1]
        if mode == "backward":
            return timed(lambda: m.train_backward(b))[1]
        if mode == "sync1":
            def phases():
                part, n = m.train_sync_begin(b, B, 0)
                while n:
                    part, n = m.train_sync_next(part[:n].unsqueeze(0))
            return timed(phases)[1]
        total, outs = 0.0, [None] * G
        for r in range(1, G):
            outs[r] = ms_[r].train_sync_begin(shard(b, r), B, r * Bl)
        torch.cuda.synchronize()
        outs[0], t = timed(lambda: m.train_sync_begin(shard(b, 0), B, 0))
        total += t
        while outs[0][1]:
            n = outs[0][1]
            parts = torch.stack([p[:n] for p, _ in outs])
            for r in range(1, G):
                outs[r] = ms_[r].train_sync_next(parts)
            torch.cuda.synchronize()
            outs[0], t = timed(lambda: m.train_sync_next(parts))
            total += t
        return total

    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ms = [call() for _ in range(reps)]
    rec = {"shape": SHAPE, "mode": mode, "deterministic": int(det), "B": B, "L": L, "ranks": G, "device": torch.cuda.get_device_name(0),
           "call_ms": _stats(ms)}
    for m in ms_:
        m.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--lookup", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_sync_bn.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        mode, det = a.child.split("/")
        return child(mode, int(det), a.batch, a.lookup, a.reps)
    import numpy as np
    jobs = []
    for det in (0, 1):
        for mode in ("step", "backward"):
            for _ in range(a.rounds):      # the two libraries alternate
                jobs += [(a.lib, mode, det)] if a.lib else []
                jobs += [("", mode, det)]
        jobs += [("", "sync1", det), ("", "rank8", det)]
    jobs += [(a.lib, "bits", 1), ("", "bits", 1)] if a.lib else []
    res = []
    for lib, mode, det in jobs:
        env = dict(os.environ)
        if lib:
            env["COPER_HIP_LIB"] = os.path.abspath(lib)
        who = "parent" if lib else "this tree"
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%s/%d" % (mode, det), "--reps", str(a.reps),
                                "--batch", str(a.batch), "--lookup", str(a.lookup)], env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:      # a hung child: its row says so, the rows so far are kept, nothing more is started
            res.append({"mode": mode, "deterministic": det, "failed": "timeout", "library": who})
            print(json.dumps(res[-1]), flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        rec = json.loads(line[-1]) if r.returncode == 0 and line else {"mode": mode, "deterministic": det, "failed": r.returncode,
                                                                        "stderr": r.stderr[-400:]}
        rec["library"] = who
        res.append(rec)
        print(json.dumps(rec), flush=True)
        if r.returncode not in (0, 1):      # (a child that died of a signal: nothing more is started on the device)
            break
    summary = []
    for det in (0, 1):
        row = {"deterministic": det}
        rows = [r for r in res if r.get("deterministic") == det and "call_ms" in r]
        for mode in ("step", "backward", "sync1", "rank8"):
            mine = [r for r in rows if r["mode"] == mode and r["library"] == "this tree"]
            theirs = [r for r in rows if r["mode"] == mode and r["library"] == "parent"]
            if mine:
                row[mode + "_ms"] = {"median": float(np.median([r["call_ms"]["median"] for r in mine])),
                                     "min": min(r["call_ms"]["min"] for r in mine), "max": max(r["call_ms"]["max"] for r in mine)}
            if mine and theirs:
                lo, hi = min(r["call_ms"]["min"] for r in theirs), max(r["call_ms"]["max"] for r in theirs)
                row["parent_" + mode + "_ms"] = {"median": float(np.median([r["call_ms"]["median"] for r in theirs])), "min": lo, "max": hi}
                row[mode + "_median_within_parent_min_max"] = bool(lo <= row[mode + "_ms"]["median"] <= hi)
        if "sync1_ms" in row and "backward_ms" in row:
            row["sync1_minus_backward_ms"] = row["sync1_ms"]["median"] - row["backward_ms"]["median"]
        bits = [r["sha256"] for r in res if r.get("mode") == "bits" and "sha256" in r]
        if det == 1 and len(bits) == 2:
            row["deterministic_bits_equal_parent"] = bits[0] == bits[1]
        summary.append(row)
    doc = {"tool": "tools/bench_train_sync.py", "shape": SHAPE, "B": a.batch, "L": a.lookup, "reps": a.reps,
           "clock": "host perf_counter around the calls + a device synchronisation; warm (5 calls); a fresh process per row; rank8: a "
                    "synchronisation behind every one of rank 0's five calls, their sum",
           "not_measured": "the four all-gathers per micro-batch over real RCCL (a few hundred bytes each); multi-GPU scaling",
           "results": res, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
