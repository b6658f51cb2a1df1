#!/usr/bin/env python3
"""Every kind of training call, twice, on the smallest shapes at which every route of coper_train.hip is taken -- the check that a
host-side change launches what the build before it launched and leaves the same bits.

    python tools/train_call_kinds.py --list                      the kinds, one per line
    python tools/train_call_kinds.py --kind KIND [--d 32,30]     runs the kind on a fresh state per d: one line per state,
                                                                 `KIND d=32 sha256=...` over the loss of every call, every gradient,
                                                                 variable and optimizer slot (and the deferred-rows statistics)
    python tools/train_call_kinds.py --compare DIR_A DIR_B       DIR_X/KIND/ holds a `rocprofv3 --kernel-trace --output-format csv`
                                                                 of `--kind KIND` on build X, DIR_X/KIND.txt what it printed

The library is the one COPER_HIP_LIB names (coper_amd/_lib.py).  Shapes: num_ent = 300, B = 16, L = 7, d = 32 and d = 30 (no 16-byte
rows: the scalar routes), one_vs_all_chunk = 128 (three CSR chunks; one full and one ragged chunk per shard), shards [0, 150) and
[150, 300) as two handles of the process, the ranks of a synchronised step likewise with the gather done by hand (torch.stack in rank
order, as tests/test_gpu_train_sync.py).  --compare asks, per kind: the same multiset of (kernel, grid, workgroup, LDS bytes); on
every deterministic and sharded state the same sequence and the same sha256 lines.  It prints one line per kind and exits 1 if any
differs.  Nothing here is tried twice."""
import argparse
import collections
import csv
import glob
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

E, B, L, CHUNK, BOUNDS = 300, 16, 7, 128, ((0, 150), (150, 300))
SHAPE = {32: (8, 4), 30: (6, 5)}      # d -> the image emb_h x emb_w


def _md(d, **over):
    from tests import test_gpu_train_deterministic as D
    md = D._md("cpg_linear")
    md.update(num_ent=E, ent_emb_size=d, emb_h=SHAPE[d][0], emb_w=SHAPE[d][1])
    md.update(over)
    return md


def _batch(md, form, k, n=B):
    from tests import test_gpu_train_deterministic as D
    return D._batch(md, form, n, L, 1000 + k)


def _handle(md, det=False, ordered=False, deferred=False):
    from tests import train_history_common as TH
    return TH.new_handle(md, (TH.p0_for(md), None), TH.mode_of(det, ordered, deferred))


def _shards(md, deferred=False):
    import torch
    from coper_amd import data as cdata
    from coper_amd.models import ConvE
    from tests import shard_train_common as SC
    p0 = SC.host_params(cdata.synthetic_params(md, seed=21, ent_std=0.1))
    ms = []
    for lo, hi in BOUNDS:
        m = ConvE(md, device="cuda:0", shard=(lo, hi))
        m.load_parameters({k: torch.as_tensor(v) for k, v in p0.items()})
        m.train_init(seed=SC.SEED, clip_norm=SC.CLIP_OFF, deterministic=True, entity_sharded=True, one_vs_all_chunk=CHUNK, deferred_rows=deferred)
        ms.append(m)
    return ms


def _host(t):
    return t.cpu().numpy().copy()


# ---- the kinds: f(d) -> ({name: host array}, [handles]).  Two calls each, on batches 0 and 1.
def _steps(form, **mode):
    def run(d):
        md = _md(d)
        m = _handle(md, **mode)
        out = {}
        for k in range(2):
            out["loss%d" % k] = _host(m.train_step(_batch(md, form, k)))
        return out, [m]
    return run


def _forwards(d):
    md = _md(d)
    m = _handle(md)
    out = {}
    for k in range(2):
        loss, pred, hv = m.train_forward(_batch(md, "sampled", k), want_predictions=True, want_h=True)
        out.update({"loss%d" % k: _host(loss), "pred%d" % k: _host(pred), "h%d" % k: _host(hv)})
    return out, [m]


def _split(flat):
    def run(d):
        md = _md(d)
        m = _handle(md)
        out = {}
        for k in range(2):
            out["loss%d" % k] = _host(m.train_backward(_batch(md, "sampled", k)))
            if flat:
                v = m.train_grads_export()
                out["flat%d" % k] = _host(v)
                m.train_apply(v, scale=0.5)
            else:
                m.train_apply()
        return out, [m]
    return run


def _rows_split(d):
    from tests import train_history_common as TH
    md = _md(d)
    m = _handle(md, deferred=True)
    out = {}
    for k in range(2):
        part = {}
        out["loss%d" % k] = _host(TH._rows_group(m, _batch(md, "sampled", k), True, 0.5, part))
        out.update({"%s/%d" % (key, k): v for key, v in part.items()})
    return out, [m]


def _sharded(form, deferred=False, forward=False):
    def run(d):
        from coper_amd.parallel import EntityShardedTrainer
        md = _md(d)
        ms = _shards(md, deferred)
        tr = EntityShardedTrainer(models=ms)
        out = {}
        if forward:      # behind one step: in the deferred-rows mode the rows it did not name are an update behind
            out["loss"] = _host(tr.step(_batch(md, form, 2)))
        for k in range(2):
            if not forward:
                out["loss%d" % k] = _host(tr.step(_batch(md, form, k)))
                continue
            loss, pred, hv = tr.forward(_batch(md, form, k), want_predictions=True, want_h=True)
            out.update({"loss%d" % k: _host(loss), "h%d" % k: _host(hv)})
            for r, p in enumerate(pred if isinstance(pred, list) else [pred]):
                out["pred%d/%d" % (k, r)] = _host(p)
        return out, ms
    return run


def _sync(det, rows=False, stats=True):
    def run(d):
        from coper_amd.parallel import shard_batch
        from tests.test_gpu_train_sync import _sync_backward
        md = _md(d, batch_norm_train_stats=stats)
        G = 2 if stats else 1
        ms = [_handle(md, det=det, ordered=rows, deferred=rows) for _ in range(G)]
        out = {}
        for k in range(2):
            whole = _batch(md, "sampled", k, G * B)
            if not stats:      # nothing to exchange: the begin call is the whole backward
                part, n = ms[0].train_sync_begin(whole, B, 0)
                assert n == 0
                out["loss%d" % k] = _host(ms[0].train_sync_loss)
                ms[0].train_apply()
                continue
            losses, _ = _sync_backward(ms, [shard_batch(whole, r, G) for r in range(G)], rows=rows)
            for r, m in enumerate(ms):
                out["loss%d/%d" % (k, r)] = _host(losses[r])
            if rows:      # export / import / apply as DataParallelTrainer._step_rows makes them
                ex = [m.train_rows_export() for m in ms]
                small = ex[0][0] + ex[1][0]
                for m in ms:
                    for r in range(G):
                        m.train_rows_import(ex[r][1], ex[r][2], first=r == 0)
                    m.train_rows_apply(small, 1.0 / G)
            else:
                flat = None
                for m in ms:
                    flat = m.train_grads_export(flat, accumulate=flat is not None)
                out["flat%d" % k] = _host(flat)
                for m in ms:
                    m.train_apply(flat, 1.0 / G)
        return out, ms
    return run


# name -> (run, the bits are defined: a deterministic or sharded state)
KINDS = collections.OrderedDict([
    ("default_step_sampled", (_steps("sampled"), False)),
    ("default_forward_sampled", (_forwards, False)),
    ("default_step_dense", (_steps("dense"), False)),
    ("default_step_csr", (_steps("csr"), False)),
    ("default_split_buffers", (_split(False), False)),
    ("default_split_flat", (_split(True), False)),
    ("det_step_sampled", (_steps("sampled", det=True), True)),
    ("det_ordered", (_steps("sampled", det=True, ordered=True), True)),
    ("det_ordered_deferred", (_steps("sampled", det=True, ordered=True, deferred=True), True)),
    ("deferred_step", (_steps("sampled", deferred=True), False)),
    ("deferred_split", (_rows_split, False)),
    ("sharded_csr", (_sharded("csr"), True)),
    ("sharded_sampled", (_sharded("sampled"), True)),
    ("sharded_sampled_deferred", (_sharded("sampled", deferred=True), True)),
    ("sharded_forward_csr", (_sharded("csr", forward=True), True)),
    ("sharded_forward_sampled", (_sharded("sampled", forward=True), True)),
    ("sharded_forward_sampled_deferred", (_sharded("sampled", deferred=True, forward=True), True)),
    ("sync_default", (_sync(False), False)),
    ("sync_det", (_sync(True), True)),
    ("sync_rows", (_sync(True, rows=True), True)),
    ("sync_stats_off", (_sync(True, stats=False), True)),
])


def run_kind(kind, ds):
    import numpy as np
    import torch
    from tests.test_gpu_train_ordered import _outs
    for d in ds:
        out, ms = KINDS[kind][0](d)
        for r, m in enumerate(ms):
            out.update({"%d/%s" % (r, k): v for k, v in _outs(m, torch.zeros(1)).items() if k != "loss"})
            m.close()
        h = hashlib.sha256()
        for k in sorted(out):
            a = np.ascontiguousarray(out[k])
            h.update(("%s %s %s " % (k, a.dtype, a.shape)).encode())
            h.update(a.tobytes())
        print("%s d=%d sha256=%s" % (kind, d, h.hexdigest()), flush=True)


def _launches(d):
    """[(kernel, grid, workgroup, LDS bytes)] of the one trace under d, in start order."""
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("%s: %d kernel traces" % (d, len(files)))
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    if not rows or any(c not in rows[0] for c in ("Grid_Size_X", "Workgroup_Size_X", "LDS_Block_Size")):
        raise SystemExit("%s: no launches, or not the columns of a kernel trace" % files[0])
    dims = lambda r, what: tuple(int(float(r.get("%s_Size_%s" % (what, a)) or 0)) for a in "XYZ")
    return [(r["Kernel_Name"], dims(r, "Grid"), dims(r, "Workgroup"), int(float(r.get("LDS_Block_Size") or 0))) for r in rows]


def compare(dir_a, dir_b):
    bad = 0
    for kind, (_, defined) in KINDS.items():
        la, lb = _launches(os.path.join(dir_a, kind)), _launches(os.path.join(dir_b, kind))
        ta, tb = ([ln.split() for ln in open(os.path.join(x, kind + ".txt")) if ln.startswith(kind + " d=")] for x in (dir_a, dir_b))
        multiset = collections.Counter(la) == collections.Counter(lb)
        res = ["launches %d %d" % (len(la), len(lb)), "multiset " + ("same" if multiset else "DIFFERS")]
        ok = multiset and len(ta) == len(tb) == 2      # (a line per state)
        if defined:
            res += ["sequence " + ("same" if la == lb else "DIFFERS"), "bits " + ("same" if ta == tb else "DIFFER")]
            ok = ok and la == lb and ta == tb
        if not multiset:
            diff = (collections.Counter(la) - collections.Counter(lb)) + (collections.Counter(lb) - collections.Counter(la))
            res.append("e.g. %r" % (sorted(diff.items())[:2],))
        print("%-34s %s" % (kind, "; ".join(res)))
        bad += not ok
    print("kinds: %d, different: %d" % (len(KINDS), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--kind", choices=list(KINDS))
    ap.add_argument("--d", default="32,30")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    a = ap.parse_args()
    if a.list:
        print("\n".join(KINDS))
    elif a.compare:
        sys.exit(compare(*a.compare))
    elif a.kind:
        run_kind(a.kind, [int(x) for x in a.d.split(",")])
    else:
        ap.error("one of --list, --kind, --compare")


if __name__ == "__main__":
    main()
