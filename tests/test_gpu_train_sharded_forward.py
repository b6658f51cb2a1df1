"""GPU tests of the forward-only calls on an entity-sharded training state (include/coper_hip.h "Entity-sharded training": "Forward-only
calls", coper_train_shard_forward_lookup / coper_train_shard_forward_csr; coper_amd.parallel.EntityShardedTrainer.forward).

What must hold:
  1. a world of one (a shard [0, num_ent)) returns the bits of `train_forward` on a deterministic whole-table handle with ordered rows:
     loss, logits and h, before any step and after two;
  2. on any sharding the summed pred [B, L] and h are that handle's bit for bit, every pred_part is +0.0f where its rank owns nothing,
     and the float32 loss is within one ulp (two orders of one sum of fewer than 1e6 doubles differ by at most n 2^-53 relative -- far
     below half a float ulp -- so the rounding moves by one step at most); the 1-vs-all blocks concatenated are the whole-table logits;
  3. a shard that owns nothing of a batch hands out an exact 0.0 and zeros;
  4. nothing is written: a run with forwards between its steps leaves the bytes of a run without them;
  5. deferred rows: the table, the words and what a later sync makes of the slots keep their bytes, and the scores are those of a twin
     that synced first;
  6. the state machine and the refusals;  7. two processes see what the in-process form sees.

The library hands out no raw slot bytes of a table in the deferred-rows mode (coper_train_slot syncs first; tests/
test_gpu_train_sharded_deferred.py), so "the slots keep their bytes" is checked by what a later sync makes of them: a slot decayed early
gives other bits than one decayed once over the whole gap (the planted slots move p by about 1e-3 per missed update)."""
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

from tests import shard_train_common as SC
from tests import shard_train_deferred_child as DC
from tests import shard_train_forward_child as FC
from tests.shard_train_sampled_child import sampled_edge_batch
from tests.test_gpu_train_sharded_sampled import _BOUNDS700, _EDGES300, _EDGES700, _close, _p0, _trainer, _whole

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIMIT = 150.0      # seconds for the ranks of one run (init_process_group itself gives up after 60)
EINVAL, ESTATE, EUNSUPPORTED = 1, 5, 7


def _np(t):
    return t.cpu().numpy().copy()


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), (what, int(np.count_nonzero(a != b)), float(np.abs(a.astype(np.float64) - b).max()))


def _ulps(a, b):
    """The distance of two positive float32 in steps of the format."""
    a, b = np.float32(a), np.float32(b)
    assert a > 0 and b > 0
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def _clamped_lookup(batch, E):
    lk = np.array(batch["lookup_values"], np.int64)
    lk[(lk < 0) | (lk >= E)] = 0
    return lk


def _assert_every_rank_owns_some_and_none(batch, E, bounds):
    """The inputs are not vacuous: every rank owns at least one entry of some sample and none of some other sample."""
    lk = _clamped_lookup(batch, E)
    for lo, hi in bounds:
        own = ((lk >= lo) & (lk < hi)).any(axis=1)
        assert own.any() and not own.all(), (lo, hi)


def _parts(tr, ms, batch, pred=True, hv=True):
    """The forward-only call of every shard by itself: [(loss_part, pred_part, h)] in rank order."""
    rows = tr._exchange([m.train_shard_gather(batch["e1"]) for m in ms], reduce=True)
    return [m.train_shard_forward_only(batch, r, pred, hv) for m, r in zip(ms, rows)]


# ------------------------------------------------------------------------------------------------ 1
def _world_of_one(md, batches, csr=False):
    """`batches`: [forward batch, step batch, step batch, forward batch] -- looked at before any step and after two."""
    p0 = _p0(md)
    E = md["num_ent"]
    w = _whole(md, p0, SC.CLIP_OFF)
    tr, ms = _trainer(md, p0, ((0, E),), SC.CLIP_OFF)
    for when, b in (("fresh", batches[0]), ("after two steps", batches[3])):
        lw, pw, hw = w.train_forward(b, want_predictions=True, want_h=True)
        lg, pg, hg = tr.forward(b, True, True)
        if csr:
            assert isinstance(pg, list) and len(pg) == 1      # (1-vs-all: the blocks in rank order, nothing exchanged)
            pg = pg[0]
        print("%s: loss %.9g (whole table %.9g)" % (when, float(lg[0]), float(lw[0])))
        assert tuple(pg.shape) == (len(b["e1"]), E if csr else b["lookup_values"].shape[1])
        assert np.isfinite(_np(pg)).all() and float(lg[0]) > 0.0 and np.count_nonzero(_np(hg)) > 0
        _same(_np(lg), _np(lw), when + " loss")
        _same(_np(pg), _np(pw), when + " pred")
        _same(_np(hg), _np(hw), when + " h")
        if when == "fresh":
            for sb in batches[1:3]:
                _same(_np(tr.step(sb)), _np(w.train_step(sb)), "step loss")
    _close(ms + [w])


def test_a_world_of_one_is_the_whole_table_handle_bit_for_bit():
    """E = 300, B = 48, L = 30, cpg_linear: the fused scorer."""
    md = SC.md_for("cpg_linear", SC.E300)
    _world_of_one(md, [sampled_edge_batch(md, 48, 30, s, _EDGES300) for s in (5, 0, 1, 6)])


def test_a_world_of_one_on_the_scalar_routes():
    """d = 77 and B = 47: k_tr_score_loss and the scalar loads; B d is no multiple of 4."""
    md = SC.md_for("cpg_linear", SC.E300, ent_emb_size=77, emb_h=7, emb_w=11)
    assert (47 * 77) % 4 != 0
    _world_of_one(md, [sampled_edge_batch(md, 47, 30, s, _EDGES300) for s in (5, 0, 1, 6)])


def test_a_world_of_one_from_sparse_labels():
    """SC.batch300 at one_vs_all_chunk = 128: loss and pred [B, 300] against `train_forward` on sparse labels, three chunks."""
    md = SC.md_for("cpg_linear", SC.E300)
    _world_of_one(md, [SC.batch300(md, s) for s in (5, 0, 1, 6)], csr=True)


# ------------------------------------------------------------------------------------------------ 2
def _edge_batch_any_sharding(md, B, L, step, edges):
    """sampled_edge_batch with sample 2 WHOLLY on the table's last row (the batch's last column is row 7 in every other sample), so that
    the rank that holds row 7 owns nothing of one sample too."""
    b = sampled_edge_batch(md, B, L, step, edges)
    b["lookup_values"][2, :] = edges[-1]
    return b


@pytest.mark.parametrize("name,E,bounds,L,edges", [("cpg_linear", SC.E300, SC.BOUNDS300, 30, _EDGES300), ("cpg_wide", 700, _BOUNDS700, 150, _EDGES700)],
                         ids=["e300", "e700"])
def test_any_sharding_sums_to_the_whole_table_logits(name, E, bounds, L, edges):
    """E = 700: cpg_wide, d = 200, L = 150 -- three row batches of the fused scorer."""
    md = SC.md_for(name, E)
    p0 = _p0(md)
    B = 48
    batch = _edge_batch_any_sharding(md, B, L, 3, edges)
    _assert_every_rank_owns_some_and_none(batch, E, bounds)
    lk = _clamped_lookup(batch, E)
    assert (np.array(batch["lookup_values"]) != lk).sum() == 4      # (the ids outside [0, E) are in: they clamp to row 0)
    for lo, hi in bounds[1:]:
        assert (lk == lo - 1).any() and (lk == lo).any()      # (both sides of every bound)
    w = _whole(md, p0, SC.CLIP_OFF)
    lw, pw, hw = w.train_forward(batch, want_predictions=True, want_h=True)
    tr, ms = _trainer(md, p0, bounds, SC.CLIP_OFF)
    lg, pg, hg = tr.forward(batch, True, True)
    _same(_np(pg), _np(pw), "summed pred")
    _same(_np(hg), _np(hw), "h")
    print("loss %.9g (whole table %.9g): %d ulp" % (float(lg[0]), float(lw[0]), _ulps(_np(lg)[0], _np(lw)[0])))
    assert _ulps(_np(lg)[0], _np(lw)[0]) <= 1
    outs = _parts(tr, ms, batch)
    total = 0.0
    for (lo, hi), (lp, pp, hp) in zip(bounds, outs):
        own = (lk >= lo) & (lk < hi)
        pp = _np(pp)
        assert pp[~own].tobytes() == np.zeros(int((~own).sum()), np.float32).tobytes(), (lo, hi)      # +0.0f, by its bytes
        _same(pp[own], _np(pw)[own], "owned logits of [%d, %d)" % (lo, hi))
        _same(_np(hp), _np(hw), "h of [%d, %d)" % (lo, hi))
        total += float(lp[0])
    _same(np.float32(total * (1.0 / (float(B) * float(L)))), _np(lg)[0], "the loss is the doubles in rank order")
    _close(ms + [w])


def test_any_sharding_concatenates_to_the_whole_table_logits_from_sparse_labels():
    """BOUNDS300 at one_vs_all_chunk = 128: every shard is one chunk of the whole-table walk."""
    md = SC.md_for("cpg_linear", SC.E300)
    p0 = _p0(md)
    batch = SC.batch300(md, 3)
    w = _whole(md, p0, SC.CLIP_OFF)
    lw, pw, hw = w.train_forward(batch, want_predictions=True, want_h=True)
    tr, ms = _trainer(md, p0, SC.BOUNDS300, SC.CLIP_OFF)
    lg, pg, hg = tr.forward(batch, True, True)
    assert isinstance(pg, list) and [tuple(p.shape) for p in pg] == [(48, hi - lo) for lo, hi in SC.BOUNDS300]
    _same(np.concatenate([_np(p) for p in pg], axis=1), _np(pw), "concatenated pred")
    _same(_np(hg), _np(hw), "h")
    print("loss %.9g (whole table %.9g)" % (float(lg[0]), float(lw[0])))
    assert _ulps(_np(lg)[0], _np(lw)[0]) <= 1
    _close(ms + [w])


# ------------------------------------------------------------------------------------------------ 3
def test_a_shard_that_owns_nothing_of_a_batch():
    """E = 300 as BOUNDS300 with every lookup id below 128: shards 1 and 2 hand out an exact 0.0 and +0.0f everywhere."""
    md = SC.md_for("cpg_linear", SC.E300)
    E = SC.E300
    batch = sampled_edge_batch(md, 48, 30, 0, _EDGES300)
    lk = batch["lookup_values"]
    batch["lookup_values"] = np.where((lk >= 0) & (lk < E), lk % 128, lk).astype(np.int32)      # (the four ids outside [0, E) stay: row 0)
    assert _clamped_lookup(batch, E).max() < 128
    tr, ms = _trainer(md, _p0(md), SC.BOUNDS300, SC.CLIP_OFF)
    outs = _parts(tr, ms, batch)
    assert float(outs[0][0][0]) > 0.0 and np.count_nonzero(_np(outs[0][1])) > 0
    for g in (1, 2):
        assert _np(outs[g][0]).tobytes() == np.zeros(1, np.float64).tobytes(), g
        assert _np(outs[g][1]).tobytes() == np.zeros((48, 30), np.float32).tobytes(), g
    loss, pred, _ = tr.forward(batch, True)
    _same(_np(pred), _np(outs[0][1]), "the sum is rank 0's part")
    _same(np.float32(float(outs[0][0][0]) * (1.0 / (48.0 * 30.0))), _np(loss)[0], "loss")
    _close(ms)


# ------------------------------------------------------------------------------------------------ 4
def test_nothing_is_written_and_training_does_not_notice():
    """A: step, step, step.  B: step, forward(another batch), forward(sparse labels), step, forward, step."""
    md = SC.md_for("cpg_linear", SC.E300)
    p0 = _p0(md)
    steps = [sampled_edge_batch(md, 48, 30, s, _EDGES300) for s in range(3)]
    other, csr = sampled_edge_batch(md, 48, 30, 7, _EDGES300), SC.batch300(md, 0)

    def after_step(ms, loss, out):
        snap = SC.snapshot(ms)
        snap["loss"] = _np(loss)
        snap["norm"] = np.float64(ms[0].train_grad("pred_bias")[1])
        out.append(snap)

    tr_a, ms_a = _trainer(md, p0, SC.BOUNDS300, SC.CLIP_OFF)
    a = []
    for b in steps:
        after_step(ms_a, tr_a.step(b), a)
    _close(ms_a)

    tr_b, ms_b = _trainer(md, p0, SC.BOUNDS300, SC.CLIP_OFF)
    got = []
    after_step(ms_b, tr_b.step(steps[0]), got)
    leaves = SC.TABLES + tuple(leaf for leaf in ms_b[0].trainable_leaves() if leaf not in SC.TABLES)[:1]      # the tables and a replicated leaf
    assert len(leaves) == 3
    grads = [[_np(m.train_grad(leaf)[0]) for leaf in leaves] for m in ms_b]
    norm = ms_b[0].train_grad("pred_bias")[1]
    before = SC.snapshot(ms_b)
    seen = tr_b.forward(other, True, True)
    SC.same_bits(before, SC.snapshot(ms_b), "around one forward")
    for m, g in zip(ms_b, grads):      # (what the last step left for coper_train_grad is still there, the global norm included)
        for leaf, want in zip(leaves, g):
            got_g, got_n = m.train_grad(leaf)
            _same(_np(got_g), want, "gradient of " + leaf)
            assert got_n == norm
    assert np.count_nonzero(grads[0][0]) > 0
    again = tr_b.forward(other, True, True)      # (the same call twice: the same bits -- no counter moved)
    for x, y, what in zip(seen, again, ("loss", "pred", "h")):
        _same(_np(x), _np(y), "repeated forward: " + what)
    loss_c, pred_c, _ = tr_b.forward(csr, True)
    assert float(loss_c[0]) > 0.0 and len(pred_c) == 3
    after_step(ms_b, tr_b.step(steps[1]), got)
    tr_b.forward(steps[2])
    after_step(ms_b, tr_b.step(steps[2]), got)
    _close(ms_b)
    for i, (g, w) in enumerate(zip(got, a)):
        SC.same_bits(g, w, "step %d" % i)


# ------------------------------------------------------------------------------------------------ 5
def _dtrainer(md, p0, planted):
    from coper_amd.parallel import EntityShardedTrainer
    ms = [DC.deferred_shard(md, p0, lo, hi, SC.CLIP_OFF, planted=planted) for lo, hi in _BOUNDS700]
    return EntityShardedTrainer(models=ms), ms


def _raw(ms):
    """The registered table tensors as they stand (NO sync) and the row words' statistics."""
    torch.cuda.synchronize()
    out = {k: np.concatenate([m._tensors[k].cpu().numpy().reshape(m.shard[1] - m.shard[0], -1) for m in ms]) for k in SC.TABLES}
    for g, m in enumerate(ms):
        for k, v in m.train_row_stats().items():
            out["stats%d/%s" % (g, k)] = np.int64(v)
        out["updates%d" % g] = np.int64(m.train_rows_updates)
    return out


@pytest.mark.parametrize("over,N", [({}, 1), ({}, 9), (dict(ent_emb_size=77, emb_h=7, emb_w=11), 9)], ids=["fused-1", "fused-9", "scalar-9"])
def test_deferred_rows_are_scored_as_of_the_current_update_and_stay_behind(over, N):
    """E = 700 as (0, 384), (384, 700), B = 8, L = 12: a step names about a hundred rows, most stay behind.  cpg_wide (d = 200) takes the
    fused scorer's CURRENT form, d = 77 k_tr_score_loss's."""
    E, B, L = 700, 8, 12
    md = SC.md_for("cpg_wide" if not over else "cpg_linear", E, **over)
    p0, planted = _p0(md), DC.planted_slots(md)
    steps = [DC.schedule_batch(md, B, L, s) for s in range(N + 2)]
    last = np.full(E, -1)
    for i in range(N):
        last[DC.named_rows(steps[i], E)[0]] = i
    gap = np.where(last >= 0, N - 1 - last, N)      # a row named by step i is current as of update i + 1; a row never named as of update 0
    never, fresh = np.nonzero(last < 0)[0], np.nonzero(gap == 0)[0]
    assert (gap > 0).sum() > E // 2 and len(never) > 100      # (most rows are behind, many were never named)
    pool = np.unique(np.concatenate([[0], never[::5], fresh[::2], np.nonzero((gap > 0) & (last >= 0))[0][::3]]))
    batch2 = DC.pool_batch(md, B, L, 7700 + N, pool)
    batch2["lookup_values"][5, :] = pool[pool >= 384][:L]      # a sample of which rank 0 owns nothing
    batch2["lookup_values"][6, :] = pool[pool < 384][:L]       # ... and rank 1
    _assert_every_rank_owns_some_and_none(batch2, E, _BOUNDS700)
    scored = np.unique(_clamped_lookup(batch2, E))
    assert (gap[scored] == 0).any() and gap[scored].max() == N and (N == 1 or (gap[scored] > 1).any())
    assert (last[scored] < 0).any() and (scored < 384).any() and (scored >= 384).any()      # (rows no step named; both sides of the bound)
    csr = SC.edge_batch(md, B, 2, _EDGES700)

    tr_a, ms_a = _dtrainer(md, p0, planted)
    for b in steps[:N]:
        tr_a.step(b)
    before = _raw(ms_a)
    for g in range(2):      # (the host's account of the words is the device's)
        lo, hi = _BOUNDS700[g]
        assert before["stats%d/max_gap" % g] == gap[lo:hi].max() and before["stats%d/rows_behind" % g] == (gap[lo:hi] > 0).sum()
    loss_a, pred_a, h_a = tr_a.forward(batch2, True, True)
    SC.same_bits(before, _raw(ms_a), "around the forward")

    # the twin: the same steps, every row brought current in the table, then the same call
    tr_t, ms_t = _dtrainer(md, p0, planted)
    for b in steps[:N]:
        tr_t.step(b)
    tr_t.sync_rows()
    synced = _raw(ms_t)
    behind = scored[gap[scored] > 0]
    assert (synced["ent_emb"][behind] != before["ent_emb"][behind]).any(axis=1).all()      # (the catch-up moves every row that is behind)
    assert (synced["pred_bias"][behind] != before["pred_bias"][behind]).any()
    loss_t, pred_t, h_t = tr_t.forward(batch2, True, True)
    print("N %d: loss %.9g (synced twin %.9g)" % (N, float(loss_a[0]), float(loss_t[0])))
    _same(_np(pred_a), _np(pred_t), "pred")
    _same(_np(loss_a), _np(loss_t), "loss")
    _same(_np(h_a), _np(h_t), "h")
    _close(ms_t)

    # 1-vs-all in the mode: refused by the trainer and by the library; the state stays usable
    with pytest.raises(ValueError, match="deferred-rows mode"):
        tr_a.forward(csr, True)
    m = ms_a[0]
    P = lambda t: C.c_void_p(t.data_ptr())
    e1, rel = m._ids(csr["e1"]), m._ids(csr["rel"])
    ip, ix, row = m._ids(csr["lab_indptr"]), m._ids(csr["lab_idx"]), m._ids(csr["lab_row"])
    rows, ls = torch.zeros((B, md["ent_emb_size"]), device=m.device), torch.zeros(1, device=m.device, dtype=torch.float64)
    rc = m._lib.coper_train_shard_forward_csr(m._h, P(e1), P(rel), P(rows), P(ip), P(ix), P(row), ip.numel() - 1, B, P(ls), None, None, m._stream())
    assert rc == EUNSUPPORTED and b"deferred-rows" in m._lib.coper_last_error(m._h), (rc, m._lib.coper_last_error(m._h))
    again = tr_a.forward(batch2, True, True)
    for x, y, what in zip((loss_a, pred_a, h_a), again, ("loss", "pred", "h")):
        _same(_np(x), _np(y), "forward after the refusals: " + what)
    SC.same_bits(before, _raw(ms_a), "around the refusals and the second forward")

    # run A goes on (a forward between its steps) beside a run that never looked: the same bytes behind a sync
    tr_a.step(steps[N])
    tr_a.forward(batch2)
    tr_a.step(steps[N + 1])
    tr_a.forward(steps[0], True)
    tr_a.sync_rows()
    snap_a = SC.snapshot(ms_a)
    _close(ms_a)
    tr_c, ms_c = _dtrainer(md, p0, planted)
    for b in steps:
        tr_c.step(b)
    tr_c.sync_rows()
    SC.same_bits(snap_a, SC.snapshot(ms_c), "the run with forwards against the run without")
    _close(ms_c)


def test_deferred_rows_at_the_fused_route_s_longest_sample():
    """L = 8192 at d = 40 on 300 rows as (0, 150), (150, 300): the CURRENT form of the fused scorer keeps ids, positions, the gaps' scalars
    and the flags of 8192 entries in LDS (136 KiB beside the row batch's 15), so its launch raises the kernel's dynamic-LDS limit.  Two
    small steps leave most rows behind; the scores are those of a twin that synced first, and the tables keep their bytes."""
    from coper_amd.parallel import EntityShardedTrainer
    E, bounds = SC.E300, ((0, 150), (150, 300))
    md = SC.md_for("cpg_linear", E)
    assert md["ent_emb_size"] == 40
    p0, planted = _p0(md), DC.planted_slots(md)
    steps = [DC.schedule_batch(md, 8, 12, s) for s in range(2)]
    named = np.unique(np.concatenate([DC.named_rows(b, E)[0] for b in steps]))
    assert 0 < len(named) < E // 2
    batch = sampled_edge_batch(md, 6, 8192, 4, _EDGES300[:5])
    batch["lookup_values"][2, :] = 299      # (a sample of which rank 0 owns nothing; sample 1 is wholly on row 0)
    batch["lookup_values"][1, :] = 0
    _assert_every_rank_owns_some_and_none(batch, E, bounds)
    scored = np.unique(_clamped_lookup(batch, E))
    assert np.isin(scored, named).any() and not np.isin(scored, named).all()

    def run(sync):
        ms = [DC.deferred_shard(md, p0, lo, hi, SC.CLIP_OFF, planted=planted) for lo, hi in bounds]
        tr = EntityShardedTrainer(models=ms)
        for b in steps:
            tr.step(b)
        if sync:
            tr.sync_rows()
        before = _raw(ms)
        out = [_np(x) for x in tr.forward(batch, True, True)]
        SC.same_bits(before, _raw(ms), "around the forward")
        _close(ms)
        return out, before

    (loss_a, pred_a, h_a), raw_a = run(False)
    (loss_t, pred_t, h_t), raw_t = run(True)
    assert (raw_a["ent_emb"] != raw_t["ent_emb"]).any(axis=1).sum() > E // 2      # (the sync moved most rows: they were behind)
    print("loss %.9g (synced twin %.9g)" % (float(loss_a[0]), float(loss_t[0])))
    _same(pred_a, pred_t, "pred")
    _same(loss_a, loss_t, "loss")
    _same(h_a, h_t, "h")


# ------------------------------------------------------------------------------------------------ 6
def test_state_machine_and_refusals():
    md = SC.md_for("cpg_linear", SC.E300)
    p0 = _p0(md)
    E, B, L, d = SC.E300, 48, 30, md["ent_emb_size"]
    b, c = sampled_edge_batch(md, B, L, 0, _EDGES300), SC.batch300(md, 0)
    tr, (m,) = _trainer(md, p0, ((0, E),), SC.CLIP_OFF)
    tr_u, (u,) = _trainer(md, p0, ((0, E),), SC.CLIP_OFF)      # the undisturbed twin
    lib, h = m._lib, m._h

    def refused(rc, code, *words):
        assert rc == code, (rc, code, lib.coper_last_error(h))
        for word in words:
            assert word.encode() in lib.coper_last_error(h), (word, lib.coper_last_error(h))

    dev = m.device
    e1, rel = m._ids(b["e1"]), m._ids(b["rel"])
    lk, lab = m._ids(b["lookup_values"], torch.int32), torch.as_tensor(b["e2_multi"]).to(dev)
    ip, ix, row = m._ids(c["lab_indptr"]), m._ids(c["lab_idx"]), m._ids(c["lab_row"])
    ls, pred = torch.zeros(1, device=dev, dtype=torch.float64), torch.zeros((B, L), device=dev)
    P, st = lambda t: C.c_void_p(t.data_ptr()), m._stream()
    rows = m.train_shard_gather(b["e1"])
    f_lk = lambda B_=B, L_=L, ls_=ls: lib.coper_train_shard_forward_lookup(h, P(e1), P(rel), P(rows), P(lk), P(lab), B_, L_, P(ls_) if ls_ is not None else None,
                                                                          P(pred), None, st)
    f_csr = lambda ls_=ls: lib.coper_train_shard_forward_csr(h, P(e1), P(rel), P(rows), P(ip), P(ix), P(row), ip.numel() - 1, B,
                                                             P(ls_) if ls_ is not None else None, None, None, st)

    assert f_lk() == 0 and f_csr() == 0      # between steps: served, and the phase has not moved
    m.train_shard_forward(b["e1"], b["rel"], rows)
    for call in (f_lk, f_csr):               # score expected
        refused(call(), ESTATE, "coper_train_shard_score_csr or coper_train_shard_score_lookup")
    dh, sq = torch.empty((1, B, d), device=dev), torch.empty(1, device=dev, dtype=torch.float64)
    m.train_shard_score_lookup(b, B, dh[0], ls)
    for call in (f_lk, f_csr):               # backward expected
        refused(call(), ESTATE, "coper_train_shard_backward")
    loss = _np(m.train_shard_backward(dh, ls.reshape(-1), sq))
    for call in (f_lk, f_csr):               # apply expected
        refused(call(), ESTATE, "coper_train_shard_apply")
    m.train_shard_apply(sq.reshape(-1))
    # ... and the step that the refused calls sat in is the undisturbed step
    _same(loss, _np(tr_u.step(b)), "loss of the disturbed step")
    SC.same_bits(SC.snapshot([m]), SC.snapshot([u]), "the disturbed step")

    rows = m.train_shard_gather(b["e1"])
    refused(f_lk(B_=0), EINVAL, "bad argument")
    refused(f_lk(B_=-3), EINVAL, "bad argument")
    refused(f_lk(L_=0), EINVAL, "bad argument")
    refused(f_lk(ls_=None), EINVAL, "bad argument")
    refused(f_csr(ls_=None), EINVAL, "bad argument")
    refused(lib.coper_train_shard_forward_lookup(h, P(e1), P(rel), None, P(lk), P(lab), B, L, P(ls), None, None, st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_forward_lookup(h, P(e1), P(rel), P(rows), None, P(lab), B, L, P(ls), None, None, st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_forward_csr(h, P(e1), P(rel), P(rows), None, P(ix), P(row), ip.numel() - 1, B, P(ls), None, None, st), EINVAL,
            "bad argument")
    refused(lib.coper_train_shard_forward_csr(h, P(e1), P(rel), P(rows), P(ip), P(ix), None, ip.numel() - 1, B, P(ls), None, None, st), EINVAL, "n_rows == B")
    loss32 = torch.zeros(1, device=dev)
    refused(lib.coper_train_forward(h, P(e1), P(rel), P(lk), P(lab), B, L, P(loss32), None, None, st), EUNSUPPORTED, "entity-sharded")
    assert f_lk() == 0 and f_csr() == 0
    _same(_np(tr.step(c)), _np(tr_u.step(c)), "the next step")      # (the refusals and the forwards left nothing behind)
    SC.same_bits(SC.snapshot([m]), SC.snapshot([u]), "the next step")
    torch.cuda.synchronize()
    _close([m, u])

    # the trainer: dense labels are refused in the style of `step`
    tr, ms = _trainer(md, p0, ((0, E),), SC.CLIP_OFF)
    dense = dict(e1=b["e1"], rel=b["rel"], e2_multi=np.zeros((B, E), np.float32), lookup_values=np.zeros((B, 0), np.int32))
    with pytest.raises(ValueError, match="dense e2_multi"):
        tr.forward(dense)
    with pytest.raises(ValueError, match="dense e2_multi"):
        tr.forward(dict(e1=b["e1"], rel=b["rel"], e2_multi=dense["e2_multi"]), True)
    _close(ms)


# ------------------------------------------------------------------------------------------------ 7
def _run_ranks(tmp_path, world, **args):
    """Starts `world` ranks of tests/shard_train_forward_child.py, waits for them under one time limit -> [the .npz of rank r as a dict].
    The first bad exit status ends the run; nothing is started again."""
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    procs, logs = [], []
    for r in range(world):
        cmd = [sys.executable, os.path.join(ROOT, "tests", "shard_train_forward_child.py"), "--rank", str(r), "--world", str(world), "--port",
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


def test_two_processes_see_what_the_in_process_form_sees(tmp_path):
    """E = 300 as (0, 150), (150, 300) in two processes (RCCL on two GPUs, else gloo on one) and as two handles of one process: one step,
    then a sampled and a sparse 1-vs-all forward -- loss, summed pred and h by their bytes; a rank's 1-vs-all block is its own."""
    md = SC.md_for("cpg_linear", SC.E300)
    bounds = ((0, 150), (150, 300))
    ranks = _run_ranks(tmp_path, 2, case="cpg_linear", num_ent=SC.E300, bounds=bounds, edges=_EDGES300, batch=48, labels=30, clip=SC.CLIP_ACTIVE)
    tr, ms = _trainer(md, _p0(md), bounds, SC.CLIP_ACTIVE)
    want = FC.run(tr, md, 48, 30, _EDGES300)
    _close(ms)
    assert isinstance(want["csr/pred"], list) and np.count_nonzero(want["sampled/pred"]) > 0
    for r in range(2):
        for k in ("step/loss", "sampled/loss", "sampled/pred", "sampled/h", "csr/loss"):
            _same(ranks[r][k], want[k], "rank %d %s" % (r, k))
        _same(ranks[r]["csr/pred"], want["csr/pred"][r], "rank %d csr/pred" % r)
