"""GPU tests of deferred rows on an entity shard (include/coper_hip.h "Deferred rows" / "Entity-sharded training"; DESIGN.md 6.11;
coper_amd.parallel.EntityShardedTrainer): sampled steps of a sharded table whose zeroing, norm and optimizer pass follow the batch.

What the bits must be:
  1. a shard [0, num_ent) in the mode is `train_init(deterministic=True, ordered_rows=True, deferred_rows=True)` + `train_step` on a
     whole-table handle -- loss of every step, every variable, slot, BN statistic and the row words' statistics; the norm to 1e-10
     relative (tests/test_gpu_train_sharded_sampled.py::_assert_whole_bits has the reason);
  2. on any sharding, one step from the same state: d(pred_bias), and after a sync p, m, v, v_hat of every table row no e1 names;
  3. rows no batch names keep their raw bytes, are reported N behind, and after a sync are the whole-table handle's rows bit for bit;
  4. the gather returns the row a sync would leave and writes nothing but its output;
  5. the same past one pass of the row kernels' grid and past two digit passes of the sort;
  6. with the clip active, the float64 oracle within dev <= 2 dev_dense + 1e-4 max|w| (tests/test_gpu_train_rows_edges.py), dev_dense
     the mode-off sharded trainer's deviation in the same test;
  7. the same bytes across runs, fresh handles, processes and the two trainer forms;
  8. the state machine and the refusals;  9. no dependence on a handle's call history.
Slots are planted in every row of both tables (tests/shard_train_deferred_child.py::planted_slots), so a missed update moves p by about
1e-3.  The library hands out no raw slot bytes of a table in the mode (coper_train_slot syncs first), so "the slots keep their bytes" is
checked by what a later sync makes of them: a slot decayed early gives other bits than one decayed once over the whole gap."""
import ctypes as C
import json
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from tests import shard_train_common as SC
from tests import shard_train_deferred_child as DC
from tests import split_common as S
from tests.test_gpu_train_ordered import _clamped, _small_md

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIMIT = 150.0
_BOUNDS700 = ((0, 384), (384, 700))
EINVAL, ESTATE, EUNSUPPORTED = 1, 5, 7
CLIP_ACTS = 0.1


def _p0(md):
    return cdata.synthetic_params(md, seed=21, ent_std=0.1)


def _close(ms):
    for m in ms:
        m.close()


def _whole(md, p0, clip, planted):
    """The whole-table handle of contract 1: deterministic, ordered rows, deferred rows."""
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(v) for k, v in SC.host_params(p0).items()})
    m.train_init(seed=SC.SEED, clip_norm=clip, deterministic=True, ordered_rows=True, deferred_rows=True, one_vs_all_chunk=SC.CHUNK)
    assert m.train_rows_deferred == 1
    if planted is not None:
        m.load_optimizer_state(planted)
    return m


def _trainer(md, p0, bounds, clip, planted, deferred=True):
    from coper_amd.parallel import EntityShardedTrainer
    ms = [DC.deferred_shard(md, p0, lo, hi, clip, deferred=deferred, planted=planted) for lo, hi in bounds]
    return EntityShardedTrainer(models=ms), ms


def _stats(ms):
    """The row words' statistics of all shards together: rows listed by the last step, rows behind, the largest gap."""
    st = [m.train_row_stats() for m in ms]
    return dict(rows_last_step=sum(s["rows_last_step"] for s in st), rows_behind=sum(s["rows_behind"] for s in st),
                max_gap=max(s["max_gap"] for s in st))


def _raw_tables(ms):
    """The registered table tensors as they stand: NO sync (a raw read, the caller's risk by contract -- here the point)."""
    torch.cuda.synchronize()
    return {k: np.concatenate([m._tensors[k].cpu().numpy().reshape(m.shard[1] - m.shard[0], -1) for m in ms]) for k in SC.TABLES}


def _table_rows(snap, rows):
    """p, m, v, v_hat of the given rows of both tables out of a snapshot."""
    return {k: v.reshape(len(v), -1)[rows] for k, v in snap.items() if k.split("/")[-1] in SC.TABLES and not k.startswith("power")}


# ------------------------------------------------------------------------------------------------ 1
def _world_of_one(md, B, L, steps=4):
    p0, planted = _p0(md), DC.planted_slots(md)
    batches = [DC.schedule_batch(md, B, L, step) for step in range(steps)]
    whole = _whole(md, p0, SC.CLIP_OFF, planted)
    tr, ms = _trainer(md, p0, ((0, md["num_ent"]),), SC.CLIP_OFF, planted)
    gaps = []
    for step, b in enumerate(batches):
        gaps.append(whole.train_row_stats()["max_gap"])
        lw, ls = whole.train_step(b).cpu().numpy().copy(), tr.step(b).cpu().numpy().copy()
        nw, ns = whole.train_grad("pred_bias")[1], ms[0].train_grad("pred_bias")[1]
        print("step %d loss %.9g norm %.9g (whole table %.9g)" % (step, float(ls[0]), ns, nw))
        assert ls.tobytes() == lw.tobytes(), (step, ls, lw)
        assert 0.0 < ns < SC.CLIP_OFF and nw < SC.CLIP_OFF and abs(ns - nw) <= 1e-10 * nw, (ns, nw)
    assert max(gaps) == 3, gaps      # rows fell three updates behind and were named again
    sw, ss = whole.train_row_stats(), _stats(ms)
    assert sw == ss and sw["rows_last_step"] > 0, (sw, ss)      # the row words, before the sync
    assert ms[0].train_rows_updates == whole.train_rows_updates == steps
    whole.train_sync_rows()
    tr.sync_rows()
    SC.same_bits(SC.snapshot(ms), SC.snapshot([whole]), "after the sync")
    assert _stats(ms)["rows_behind"] == 0
    _close(ms + [whole])


@pytest.mark.parametrize("name", ["cpg_linear", "plain", "lookup"])
def test_a_world_of_one_is_the_whole_table_deferred_handle(name):
    """E = 300, B = 48, L = 30, four steps of the schedule: rows fall 1, 2 and 3 updates behind and are named again."""
    _world_of_one(SC.md_for(name, SC.E300), 48, 30)


def test_a_world_of_one_on_the_scalar_routes():
    """d = 77 and B = 47: the scalar catch-up, gather, segment reduce, norm and update."""
    _world_of_one(SC.md_for("cpg_linear", SC.E300, ent_emb_size=77, emb_h=7, emb_w=11), 47, 30)


def test_a_world_of_one_over_three_row_batches():
    """cpg_wide, E = 700, d = 200, L = 150: the fused scorer walks three row batches per sample, the last one ragged."""
    md = SC.md_for("cpg_wide", 700)
    assert md["ent_emb_size"] == 200
    _world_of_one(md, 48, 150)


# ------------------------------------------------------------------------------------------------ 2
def _one_step_case(md, bounds, batch):
    """One step from the same planted state on the whole-table deferred handle and on `bounds` -> (models, trainer) still open, after
    the equalities of contract 2 held."""
    E = md["num_ent"]
    p0, planted = _p0(md), DC.planted_slots(md)
    whole = _whole(md, p0, SC.CLIP_OFF, planted)
    whole.train_step(batch)
    assert whole.train_grad("pred_bias")[1] < SC.CLIP_OFF
    want_db = whole.train_grad("pred_bias")[0].cpu().numpy().copy()
    sw = whole.train_row_stats()
    tr, ms = _trainer(md, p0, bounds, SC.CLIP_OFF, planted)
    tr.step(batch)
    got_db = np.concatenate([m.train_grad("pred_bias")[0].cpu().numpy() for m in ms])
    assert got_db.tobytes() == want_db.tobytes() and np.count_nonzero(want_db) > 0
    listed, e1 = DC.named_rows(batch, E)
    assert _stats(ms) == sw and sw["rows_last_step"] == len(listed) and sw["rows_behind"] == E - len(listed), (sw, _stats(ms), len(listed))
    for m, (lo, hi) in zip(ms, bounds):      # every shard listed its own rows of the batch
        assert m.train_row_stats()["rows_last_step"] == int(((listed >= lo) & (listed < hi)).sum())
    whole.train_sync_rows()
    tr.sync_rows()
    free = np.ones(E, bool)
    free[e1] = False
    SC.same_bits(_table_rows(SC.snapshot(ms), free), _table_rows(SC.snapshot([whole]), free), "rows no e1 names")
    whole.close()
    return tr, ms


@pytest.mark.parametrize("case", ["e300", "e700"])
def test_one_step_on_any_sharding(case):
    """128 + 128 + 44 of 300 (d = 40) and 384 + 316 of 700 (d = 200): d(pred_bias), the row statistics, and after a sync every table
    row no e1 names with its slots are the whole-table deferred handle's."""
    md, bounds, B, L = (SC.md_for("cpg_linear", SC.E300), SC.BOUNDS300, 48, 30) if case == "e300" else (SC.md_for("cpg_wide", 700), _BOUNDS700, 48, 150)
    _, ms = _one_step_case(md, bounds, DC.schedule_batch(md, B, L, 3))
    _close(ms)


def test_a_shard_that_owns_nothing_of_a_batch():
    """128 + 128 + 44 of 300 with every id of the batch below 256: the third shard's list is empty, its dh_part and loss_part are exact
    zeros, none of its words moves (all 44 rows one update behind afterwards), and its raw rows keep their bytes."""
    md = SC.md_for("cpg_linear", SC.E300)
    p0, planted = _p0(md), DC.planted_slots(md)
    batch = DC.pool_batch(md, 48, 30, 77, np.arange(256))
    tr, ms = _trainer(md, p0, SC.BOUNDS300, SC.CLIP_OFF, planted)
    before = _raw_tables(ms[2:])
    B, d = 48, md["ent_emb_size"]
    rows = tr._exchange([m.train_shard_gather(batch["e1"]) for m in ms], reduce=True)
    dh, ls, sq = [], [], []
    for m, r in zip(ms, rows):
        m.train_shard_forward(batch["e1"], batch["rel"], r)
        dh.append(torch.full((B, d), 7.0, device=m.device, dtype=torch.float32))
        ls.append(torch.full((1,), 7.0, device=m.device, dtype=torch.float64))
        sq.append(torch.full((1,), 7.0, device=m.device, dtype=torch.float64))
        m.train_shard_score_lookup(batch, B, dh[-1], ls[-1])
    assert np.count_nonzero(dh[0].cpu().numpy()) > 0 and not dh[2].cpu().numpy().any() and float(ls[2][0]) == 0.0
    dh_all, ls_all = tr._exchange(dh), tr._exchange(ls)
    for m, a, l, s in zip(ms, dh_all, ls_all, sq):
        m.train_shard_backward(a, l.reshape(-1), s)
    assert float(sq[2][0]) == 0.0 and float(sq[0][0]) > 0.0      # the empty list's norm is an exact zero
    for m, s in zip(ms, tr._exchange(sq)):
        m.train_shard_apply(s.reshape(-1))
    st = ms[2].train_row_stats()
    assert st == dict(rows_last_step=0, rows_behind=44, max_gap=1), st
    SC.same_bits(_raw_tables(ms[2:]), before, "the raw rows of the shard that owns nothing")
    SC.replicated_equal(ms)
    _close(ms)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("N,B,L", [(1, 8, 12), (9, 8, 12), (450, 4, 8)])
def test_rows_nobody_names(N, B, L):
    """N steps whose batches avoid the rows id % 3 == 2 (a third of every shard), on 128 + 128 + 44 of 300 and on the whole-table
    deferred handle.  Before the sync the raw table bytes of those rows are unchanged and every shard reports them N behind; after it
    they and their slots are the whole-table handle's bit for bit (N = 450: past the truncation window of C at beta1 = 0.9)."""
    md = SC.md_for("cpg_linear", SC.E300)
    E = SC.E300
    p0, planted = _p0(md), DC.planted_slots(md)
    ids = np.arange(E)
    idle = ids % 3 == 2
    whole = _whole(md, p0, SC.CLIP_OFF, planted)
    tr, ms = _trainer(md, p0, SC.BOUNDS300, SC.CLIP_OFF, planted)
    before = _raw_tables(ms)
    for step in range(N):
        batch = DC.pool_batch(md, B, L, 2000 + step % 16, ids[~idle])
        whole.train_step(batch)
        tr.step(batch)
    raw = _raw_tables(ms)
    for k in SC.TABLES:
        assert raw[k][idle].tobytes() == before[k][idle].tobytes(), k
        assert raw[k][~idle].tobytes() != before[k][~idle].tobytes(), k
    for m, (lo, hi) in zip(ms, SC.BOUNDS300):
        st = m.train_row_stats()
        assert st["max_gap"] == N and st["rows_behind"] >= int(idle[lo:hi].sum()) > 0, (st, N)
    whole.train_sync_rows()
    tr.sync_rows()
    assert _stats(ms)["rows_behind"] == 0
    got, want = _table_rows(SC.snapshot(ms), idle), _table_rows(SC.snapshot([whole]), idle)
    SC.same_bits(got, want, "idle rows after %d steps" % N)
    assert np.abs(got["var/ent_emb"] - before["ent_emb"][idle]).max() > 1e-4      # the catch-up moved them
    _close(ms + [whole])


# ------------------------------------------------------------------------------------------------ 4
def test_the_gather_returns_current_rows_and_writes_nothing_else():
    """150 + 150 of 300, three steps that avoid the rows id % 3 == 2; e1 names such rows of both shards (one twice), rows the last step
    brought current and an id outside the table.  The shards' gathers sum to the rows read after a sync, bit for bit; the raw tables and
    the row statistics are what they were; and a twin that never gathered ends in the same bytes (so no slot and no word moved)."""
    md = SC.md_for("cpg_linear", SC.E300)
    E, bounds = SC.E300, ((0, 150), (150, 300))
    p0, planted = _p0(md), DC.planted_slots(md)
    ids = np.arange(E)
    idle = ids % 3 == 2
    runs = []
    for gather in (True, False):
        tr, ms = _trainer(md, p0, bounds, SC.CLIP_OFF, planted)
        for step in range(3):
            tr.step(DC.pool_batch(md, 8, 12, 2000 + step, ids[~idle]))
        if gather:
            last = DC.named_rows(DC.pool_batch(md, 8, 12, 2002, ids[~idle]), E)[0]      # the rows the last step listed: gap 0
            e1 = np.array([2, 149, 152, 299, 2, last[0], last[-1], last[len(last) // 2], E + 3], np.int64)
            assert idle[e1[:5]].all() and not idle[e1[5:8]].any() and last[0] < 150 <= last[-1]
            raw, st = _raw_tables(ms), [m.train_row_stats() for m in ms]
            assert all(s["max_gap"] == 3 for s in st)
            parts = [m.train_shard_gather(e1).cpu().numpy() for m in ms]
            for p, (lo, hi) in zip(parts, bounds):      # a row of another shard (and an id outside the table) is a zero row
                assert not p[(e1 < lo) | (e1 >= hi)].any() and np.count_nonzero(p[(e1 >= lo) & (e1 < hi)]) > 0
            got = parts[0] + parts[1]
            SC.same_bits(_raw_tables(ms), raw, "the raw tables behind the gather")
            assert [m.train_row_stats() for m in ms] == st
            assert np.abs(got[:5] - raw["ent_emb"][e1[:5]]).max() > 1e-4      # behind in the table, current in the gather
            assert got[5:8].tobytes() == raw["ent_emb"][e1[5:8]].tobytes()    # gap 0: the row as it stands
        tr.sync_rows()
        snap = SC.snapshot(ms)
        if gather:
            assert got[:8].tobytes() == snap["var/ent_emb"][e1[:8]].tobytes()
        runs.append(snap)
        _close(ms)
    SC.same_bits(runs[0], runs[1], "with and without the gather")


# ------------------------------------------------------------------------------------------------ 5
def test_more_listed_rows_than_one_pass_and_three_digit_passes():
    """E = 70,000 at d = 12 as 33,333 + 36,667, B = 512, L = 400: three 8-bit digit passes, and the second shard lists more rows than
    one pass of a row kernel's grid (8,192 workgroups x 4 rows).  Step 1 from the planted state: contract 2.  Step 2 re-zeroes that
    list: afterwards every gradient row off step 2's list is zero, and the statistics are the lists' lengths."""
    E, bounds, B, L = 70000, ((0, 33333), (33333, 70000)), 512, 400
    md = _small_md(E)
    rng = np.random.default_rng(11)
    mk = lambda: dict(e1=rng.integers(0, E, B).astype(np.int64), rel=rng.integers(0, md["num_rel"], B).astype(np.int64),
                      lookup_values=rng.integers(0, E, (B, L)).astype(np.int32), e2_multi=(rng.random((B, L)) < 0.05).astype(np.float32))
    b1, b2 = mk(), mk()
    listed1, listed2 = DC.named_rows(b1, E)[0], DC.named_rows(b2, E)[0]
    assert int((listed1 >= 33333).sum()) > 8192 * 4, int((listed1 >= 33333).sum())
    tr, ms = _one_step_case(md, bounds, b1)      # (ends with a sync: every row current, the lists still owed their re-zero)
    tr.step(b2)
    on2 = np.zeros(E, bool)
    on2[listed2] = True
    assert on2[listed1].sum() < len(listed1)      # rows of step 1's list that step 2 does not name: only the re-zero clears them
    ge = np.concatenate([m.train_grad("ent_emb")[0].cpu().numpy().reshape(hi - lo, -1) for m, (lo, hi) in zip(ms, bounds)])
    gb = np.concatenate([m.train_grad("pred_bias")[0].cpu().numpy() for m in ms])
    assert not ge[~on2].any() and not gb[~on2].any() and np.count_nonzero(ge[on2]) > 0
    for m, (lo, hi) in zip(ms, bounds):
        st = m.train_row_stats()
        own = int(((listed2 >= lo) & (listed2 < hi)).sum())
        assert st == dict(rows_last_step=own, rows_behind=(hi - lo) - own, max_gap=1), (st, own)
    _close(ms)


# ------------------------------------------------------------------------------------------------ 6
def test_two_shards_with_the_clip_active_against_the_oracle():
    """E = 700 as 384 + 316, clip_norm 0.1 below every step's norm (asserted on the oracle's), six steps of the schedule with planted
    slots in the oracle too: after a sync every leaf and slot within dev <= 2 dev_dense + 1e-4 max|w| of the float64 oracle, dev_dense
    the mode-off sharded trainer's deviation on the same sharding.  Here the listed rows' share of the norm acts in every element.
    Measured: DESIGN.md 6.11."""
    from oracle import coper_train_oracle as T
    md = SC.md_for("cpg_linear", 700)
    p0, planted = _p0(md), DC.planted_slots(md)
    batches = [DC.schedule_batch(md, 8, 12, step) for step in range(6)]
    ref, opt = S.new_oracle(md, p0, clip=CLIP_ACTS)
    for leaf, (mm, vv, hh) in planted.items():
        opt.m[leaf], opt.v[leaf], opt.vh[leaf] = mm.astype(np.float64), vv.astype(np.float64), hh.astype(np.float64)
    norms = []
    for step, b in enumerate(batches):
        cb = _clamped(b, md["num_ent"])
        ob = dict(e1=cb["e1"], rel=cb["rel"], lookup=cb["lookup_values"], labels=cb["e2_multi"])
        norms.append(float(T.train_step(ref, md, ob, opt, seed=SC.SEED, step=step, momentum=md["batch_norm_momentum"])[2]))
    print("oracle norms " + " ".join("%.3f" % g for g in norms))
    assert min(norms) > 2.0 * CLIP_ACTS, norms
    want = {"var/" + k: np.asarray(v, np.float64) for k, v in ref.items()}
    for i, slot in enumerate((opt.m, opt.v, opt.vh)):
        want.update({"slot%d/%s" % (i, leaf): np.asarray(a, np.float64) for leaf, a in slot.items()})
    got = {}
    for mode in ("deferred", "dense"):
        tr, ms = _trainer(md, p0, _BOUNDS700, CLIP_ACTS, planted, deferred=mode == "deferred")
        for b in batches:
            tr.step(b)
        if mode == "deferred":
            assert _stats(ms)["max_gap"] >= 3
        tr.sync_rows()
        SC.replicated_equal(ms)
        got[mode] = SC.snapshot(ms)
        _close(ms)
    bad = []
    for key, w in sorted(want.items()):
        dev = {mode: float(np.abs(got[mode][key].astype(np.float64).reshape(w.shape) - w).max()) for mode in got}
        room = 1e-4 * float(np.abs(w).max())
        print("%-60s deferred %.3e dense %.3e room %.3e" % (key, dev["deferred"], dev["dense"], room))
        if not dev["deferred"] <= 2.0 * dev["dense"] + room:
            bad.append((key, dev, room))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 7
def _deferred_run(md, bounds, B, L, steps, clip):
    """What tests/shard_train_deferred_child.py writes, from the in-process trainer form -> the same keys over all shards."""
    tr, ms = _trainer(md, _p0(md), bounds, clip, DC.planted_slots(md))
    out = {}
    for step in range(steps):
        out["s%d/loss" % step] = tr.step(DC.schedule_batch(md, B, L, step)).cpu().numpy().copy()
        norms = [m.train_grad("pred_bias")[1] for m in ms]
        assert all(n == norms[0] for n in norms), norms
        out["s%d/norm" % step] = np.float64(norms[0])
    out["stats"] = [m.train_row_stats() for m in ms]
    out["updates"] = np.int64(ms[0].train_rows_updates)
    tr.sync_rows()
    SC.replicated_equal(ms)      # replicated leaves, their slots, the powers and the counter: byte-identical on the ranks
    assert len({m.train_rows_updates for m in ms}) == 1
    SC.snapshot(ms, out, "end/")
    _close(ms)
    return out


def _run_ranks(tmp_path, world, **args):
    """tests/test_gpu_train_sharded_sampled.py::_run_ranks for tests/shard_train_deferred_child.py: one time limit, the first bad exit
    status ends the run, nothing is started again."""
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    procs, logs = [], []
    for r in range(world):
        cmd = [sys.executable, os.path.join(ROOT, "tests", "shard_train_deferred_child.py"), "--rank", str(r), "--world", str(world), "--port",
               str(port), "--backend", backend, "--out", str(tmp_path / ("rank%d.npz" % r))]
        for k, v in args.items():
            cmd += ["--" + k.replace("_", "-"), json.dumps(v) if isinstance(v, (list, tuple, dict)) else str(v)]
        logs.append(open(str(tmp_path / ("rank%d.log" % r)), "wb"))
        procs.append(subprocess.Popen(cmd, env=env, stdout=logs[-1], stderr=subprocess.STDOUT, start_new_session=True, cwd=ROOT))
    failed, t0 = None, time.time()
    try:
        live = set(range(world))
        while live and failed is None:
            time.sleep(0.05)
            if time.time() - t0 > _LIMIT:
                failed = "ranks %s still running after %d s" % (sorted(live), _LIMIT)
                break
            for r in sorted(live):
                code = procs[r].poll()
                if code is None:
                    continue
                live.discard(r)
                if code != 0:
                    failed = "rank %d exited with code %d" % (r, code)
                    break
    finally:
        for pr in procs:
            if pr.poll() is None:
                try:
                    os.killpg(pr.pid, signal.SIGTERM)
                except ProcessLookupError:
                    pass
        for pr in procs:
            try:
                pr.wait(timeout=30)
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(pr.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                pr.wait()
        for f in logs:
            f.close()
    if failed is not None:
        tails = "\n".join("--- rank %d\n%s" % (r, open(str(tmp_path / ("rank%d.log" % r)), errors="replace").read()[-3000:]) for r in range(world))
        pytest.fail(failed + "\n" + tails)
    return [dict(np.load(str(tmp_path / ("rank%d.npz" % r)))) for r in range(world)]


def test_two_runs_from_fresh_handles_leave_the_same_bytes():
    md = SC.md_for("cpg_linear", SC.E300)
    a, b = (_deferred_run(md, SC.BOUNDS300, 48, 30, 4, CLIP_ACTS) for _ in range(2))
    assert a.pop("stats") == b.pop("stats")
    SC.same_bits(a, b, "second run")


def test_two_processes_leave_the_bits_of_the_in_process_form(tmp_path):
    """E = 300 as 150 + 150 in two processes (RCCL on two GPUs, else gloo on one) and as two handles of one process, four steps of the
    schedule with the clip active: losses, norms, row statistics, update counter, and after a sync every byte a rank holds."""
    md = SC.md_for("cpg_linear", SC.E300)
    bounds = ((0, 150), (150, 300))
    ranks = _run_ranks(tmp_path, 2, case="cpg_linear", num_ent=SC.E300, bounds=bounds, batch=48, labels=30, steps=4, clip=CLIP_ACTS)
    got = _deferred_run(md, bounds, 48, 30, 4, CLIP_ACTS)
    stats = got.pop("stats")
    for r, (lo, hi) in enumerate(bounds):
        mine = dict(ranks[r])
        assert {k[len("stats/"):]: int(mine.pop(k)) for k in list(mine) if k.startswith("stats/")} == stats[r]
        assert float(mine["s3/norm"]) > CLIP_ACTS      # (the clip acts: the gathered norm matters to every bit compared here)
        want = {k: (v[lo:hi] if k.startswith(("end/var/", "end/slot")) and k.split("/")[-1] in SC.TABLES else v) for k, v in got.items()}
        SC.same_bits(mine, want, "rank %d" % r)


# ------------------------------------------------------------------------------------------------ 8
def test_state_machine_and_refusals():
    """The switch between steps only; score_csr refused in the mode with the phase kept, score_lookup then completing the step with a
    world of one's bits; the row-block split step refused; turning the mode off leaves current tables and the never-enabled trainer's
    next step; entering the mode on a state that has stepped stays refused; prepare() and a table slot read see current rows; the
    trainer's two ValueErrors."""
    from coper_amd._lib import CoperError
    from coper_amd.parallel import EntityShardedTrainer
    md = SC.md_for("cpg_linear", SC.E300)
    E = SC.E300
    p0, planted = _p0(md), DC.planted_slots(md)
    m = DC.deferred_shard(md, p0, 0, E, SC.CLIP_OFF, planted=planted)
    lib, h = m._lib, m._h

    def refused(rc, code, *words):
        assert rc == code, (rc, code, lib.coper_last_error(h))
        for word in words:
            assert word.encode() in lib.coper_last_error(h), (word, lib.coper_last_error(h))

    b = DC.schedule_batch(md, 48, 30, 0)
    c = SC.batch300(md, 0)
    B, L, d = 48, 30, md["ent_emb_size"]
    dev = m.device
    e1, rel = m._ids(b["e1"]), m._ids(b["rel"])
    lk = m._ids(b["lookup_values"], torch.int32)
    lab = torch.as_tensor(b["e2_multi"]).to(dev)
    ip, ix, row = m._ids(c["lab_indptr"]), m._ids(c["lab_idx"]), m._ids(c["lab_row"])
    dh, ls, sq = torch.zeros((1, B, d), device=dev), torch.zeros(1, device=dev, dtype=torch.float64), torch.zeros(1, device=dev, dtype=torch.float64)
    loss = torch.zeros(1, device=dev)
    P, st = lambda t: C.c_void_p(t.data_ptr()), m._stream()
    rows = m.train_shard_gather(b["e1"])
    assert lib.coper_train_shard_forward(h, P(e1), P(rel), P(rows), B, None, st) == 0
    refused(lib.coper_train_defer_rows(h, 0, st), ESTATE, "coper_train_shard_score_csr or coper_train_shard_score_lookup")
    refused(lib.coper_train_shard_score_csr(h, P(ip), P(ix), P(row), ip.numel() - 1, B, P(dh), P(ls), st), EUNSUPPORTED, "gradient in every row")
    assert lib.coper_train_shard_score_lookup(h, P(lk), P(lab), B, L, P(dh), P(ls), st) == 0      # the phase stayed "score expected"
    refused(lib.coper_train_defer_rows(h, 0, st), ESTATE, "coper_train_shard_backward")
    assert lib.coper_train_shard_backward(h, P(dh), P(ls), 1, P(loss), P(sq), st) == 0
    refused(lib.coper_train_defer_rows(h, 1, st), ESTATE, "coper_train_shard_apply")
    assert lib.coper_train_shard_apply(h, P(sq), 1, st) == 0
    torch.cuda.synchronize()
    # ... the step's bits are a world of one's: the whole-table deferred handle after the same batch
    whole = _whole(md, p0, SC.CLIP_OFF, planted)
    lw = whole.train_step(b).cpu().numpy()
    assert loss.cpu().numpy().tobytes() == lw.tobytes()
    # what stays refused on a sharded state, in the mode too
    refused(lib.coper_train_order_rows(h, 1, st), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_rows_backward(h, P(e1), P(rel), P(lk), P(lab), B, L, P(loss), st), EUNSUPPORTED, "entity-sharded")
    small = torch.zeros(64, device=dev)
    idb, vals = torch.zeros(64, device=dev, dtype=torch.int32), torch.zeros((64, 44), device=dev)
    refused(lib.coper_train_rows_export(h, P(small), 64, 0, P(idb), P(vals), 64, None, st), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_rows_import(h, P(idb), P(vals), 1, 1, st), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_rows_apply(h, None, 0, 1.0, st), EUNSUPPORTED, "entity-sharded")
    m.train_sync_rows()
    whole.train_sync_rows()
    SC.same_bits(SC.snapshot([m]), SC.snapshot([whole]), "the step that score_csr interrupted")
    _close([m, whole])

    # prepare() and a table slot read after deferred steps see current rows; mode off after three steps: current tables without a
    # further call, and the next mode-off step is the never-enabled trainer's from that state
    bounds = ((0, 150), (150, 300))
    tr, ms = _trainer(md, p0, bounds, SC.CLIP_OFF, planted)
    for step in range(3):
        tr.step(DC.schedule_batch(md, 48, 30, step))
    assert _stats(ms)["rows_behind"] > 0
    twin_tr, twin = _trainer(md, p0, bounds, SC.CLIP_OFF, planted)
    for step in range(3):
        twin_tr.step(DC.schedule_batch(md, 48, 30, step))
    twin_tr.sync_rows()
    want = SC.snapshot(twin)
    ms[0].prepare()                                        # syncs shard 0 by itself ...
    assert ms[0].train_row_stats()["rows_behind"] == 0
    buf, n = torch.zeros(150, device=dev), C.c_int64()      # ... and a table slot read (coper_train_slot itself) shard 1
    assert ms[1]._lib.coper_train_slot(ms[1]._h, b"pred_bias", 0, P(buf), 150, 0, C.byref(n), ms[1]._stream()) == 0 and n.value == 150
    assert ms[1].train_row_stats()["rows_behind"] == 0
    assert buf.cpu().numpy().tobytes() == want["slot0/pred_bias"][150:].tobytes()
    for mm in ms:
        mm.train_defer_rows(False)
        assert mm.train_rows_deferred == 0 and mm.train_rows_updates == 0
    raw = _raw_tables(ms)
    for k in SC.TABLES:
        assert raw[k].tobytes() == want["var/" + k].reshape(E, -1).tobytes(), k
    states = [({n: v.clone() for n, v in mm._tensors.items()}, mm.optimizer_state()) for mm in ms]
    nxt = DC.schedule_batch(md, 48, 30, 3)
    loss_off = tr.step(nxt).cpu().numpy().copy()
    never = []
    for (tensors, (sl, powers)), (lo, hi) in zip(states, bounds):
        f = DC.deferred_shard(md, p0, lo, hi, SC.CLIP_OFF, deferred=False)
        f.load_parameters({k: v.clone() for k, v in tensors.items()}, global_rows=False)
        f.load_optimizer_state(sl, powers)
        never.append(f)
    loss_never = EntityShardedTrainer(models=never).step(nxt).cpu().numpy().copy()
    assert loss_off.tobytes() == loss_never.tobytes()
    SC.same_bits(SC.snapshot(ms), SC.snapshot(never), "the mode-off step after the mode")

    # entering the mode on a sharded state that has stepped is not built: the refusal such a state always gave, and nothing changes
    with pytest.raises(CoperError, match="entity-sharded") as bad:
        ms[0].train_defer_rows(True)
    assert bad.value.code == EUNSUPPORTED and ms[0].train_rows_deferred == 0
    _close(ms + twin + never)

    # the trainer: ranks that disagree on the mode or on its counter; a CSR batch in the mode
    on = [DC.deferred_shard(md, p0, lo, hi, SC.CLIP_OFF, planted=planted) for lo, hi in bounds]
    off1 = DC.deferred_shard(md, p0, 150, 300, SC.CLIP_OFF, deferred=False, planted=planted)
    with pytest.raises(ValueError, match="deferred-rows mode"):
        EntityShardedTrainer(models=[on[0], off1])
    tr2 = EntityShardedTrainer(models=on)
    with pytest.raises(ValueError, match="sampled batches only"):
        tr2.step(SC.batch300(md, 0))
    tr2.step(nxt)
    new1 = DC.deferred_shard(md, p0, 150, 300, SC.CLIP_OFF, planted=planted)      # (in the mode, its counter 0 beside rank 0's 1)
    assert (on[0].train_rows_updates, new1.train_rows_updates) == (1, 0)
    with pytest.raises(ValueError, match="update counter"):
        EntityShardedTrainer(models=[on[0], new1])
    with pytest.raises(CoperError) as bad:      # the model-level call is the library's refusal
        on[0].train_shard_forward(nxt["e1"], nxt["rel"], on[0].train_shard_gather(nxt["e1"]))
        on[0].train_shard_score(SC.batch300(md, 0), 48, torch.zeros((48, d), device=dev), torch.zeros(1, device=dev, dtype=torch.float64))
    assert bad.value.code == EUNSUPPORTED
    _close(on + [off1, new1])


# ------------------------------------------------------------------------------------------------ 9
def test_the_mode_does_not_depend_on_the_handles_history():
    """Handles with a history -- a sparse 1-vs-all step, a sampled step with a LARGER batch, prepare(), an encode and the logits of
    the shard -- start a training state in the mode (the mode is chosen before a state's first step) beside freshly created handles
    loaded with their variables, slots, powers and counter; four steps of the schedule and a sync later both hold the same bytes
    (DESIGN.md 6.9)."""
    from coper_amd.models import ConvE
    from coper_amd.parallel import EntityShardedTrainer
    from tests import train_history_common as TH
    md = SC.md_for("cpg_linear", SC.E300)
    bounds = ((0, 150), (150, 300))
    p0 = _p0(md)

    def into_the_mode(m, state):
        m.train_init(seed=SC.SEED, clip_norm=SC.CLIP_OFF, deterministic=True, entity_sharded=True, deferred_rows=True, one_vs_all_chunk=TH.CHUNK)
        m.load_optimizer_state(*state[1])
        assert m.train_rows_deferred == 1 and m.train_rows_updates == 0

    with TH.LiveBytes():
        hist = [SC.shard_model(md, p0, lo, hi, SC.CLIP_OFF, chunk=TH.CHUNK) for lo, hi in bounds]
        fresh = []
        try:
            tr = EntityShardedTrainer(models=hist)
            tr.step(TH.op_batch(md, ("C", 40), 0))
            tr.step(TH.op_batch(md, ("S", 64, 50), 1))
            q = cdata.synthetic_queries(md, 8, seed=3)
            for m in hist:      # an evaluation pass over the shard: the prepared caches, the encoder, the 1-vs-all logits
                m.prepare()
                m.score_all(m.encode(q["e1"], q["rel"], e1_rows=torch.full((8, md["ent_emb_size"]), 0.05)))
            states = [({n: v.clone() for n, v in m._tensors.items()}, m.optimizer_state()) for m in hist]
            for m, state, (lo, hi) in zip(hist, states, bounds):
                into_the_mode(m, state)
                f = ConvE(md, device="cuda:0", shard=(lo, hi))
                fresh.append(f)
                f.load_parameters({k: v.clone() for k, v in state[0].items()}, global_rows=False)
                into_the_mode(f, state)
            trs = [EntityShardedTrainer(models=hist), EntityShardedTrainer(models=fresh)]
            for step in range(4):
                b = DC.schedule_batch(md, 48, 30, step)
                lh, lf = (t.step(b).cpu().numpy().copy() for t in trs)
                assert lh.tobytes() == lf.tobytes(), (step, lh, lf)
            assert [m.train_row_stats() for m in hist] == [m.train_row_stats() for m in fresh]
            for t in trs:
                t.sync_rows()
            SC.same_bits(SC.snapshot(hist), SC.snapshot(fresh), "a history against none")
        finally:
            _close(hist + fresh)
