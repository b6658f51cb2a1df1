"""GPU tests of sampled batches on an entity-sharded training state (include/coper_hip.h "Entity-sharded training",
coper_train_shard_score_lookup; coper_amd.parallel.EntityShardedTrainer).

What the bits must be:
  1. the same state and batch give the same bits in every output -- across runs, handles, processes and the two trainer forms;
  2. a world of one (a shard [0, num_ent), the clip idle) leaves the bits of `train_init(deterministic=True, ordered_rows=True)` +
     `train_step` on a whole-table handle -- loss, variables, slots, BN statistics; the norm to 1e-10 relative, the allowance
     tests/test_gpu_train_sharded.py::_assert_single_bits derives -- also when sampled and sparse 1-vs-all steps alternate;
  3. on any sharding d(pred_bias) (shards in rank order) and every row of d(ent_emb) that no e1 of the batch names are the whole-table
     ordered handle's, bit for bit: ds and the segment sums are functions of the batch alone (the e1 rows also take the conv
     backward's share, which depends on the association of dh);
  4. otherwise the float64 oracle by the step-0 bounds: loss 2e-5 max(1, |loss|), gradients 2e-4 by _rel_err
     (split_common.check_grads), norm 1e-4 relative.

Ranks in processes of their own (tests/shard_train_sampled_child.py) are started as tests/test_gpu_train_sharded.py starts its ranks:
one time limit per run, the first bad exit status ends it, nothing is started again."""
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
from tests import split_common as S
from tests.shard_train_sampled_child import sampled_edge_batch
from tests.test_gpu_train_ordered import _clamped, _small_md

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIMIT = 150.0      # seconds for the ranks of one run (init_process_group itself gives up after 60)
_EDGES300 = (0, 127, 128, 255, 256, 299)
_EDGES700 = (0, 127, 128, 383, 384, 699)
_BOUNDS700 = ((0, 384), (384, 700))


def _p0(md):
    return cdata.synthetic_params(md, seed=21, ent_std=0.1)


def _close(ms):
    for m in ms:
        m.close()


def _whole(md, p0, clip):
    """The whole-table comparison handle: deterministic, ordered rows (CSR steps walk chunks of SC.CHUNK columns, as the shards do)."""
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(v) for k, v in SC.host_params(p0).items()})
    m.train_init(seed=SC.SEED, clip_norm=clip, deterministic=True, ordered_rows=True, one_vs_all_chunk=SC.CHUNK)
    return m


def _trainer(md, p0, bounds, clip):
    from coper_amd.parallel import EntityShardedTrainer
    ms = [SC.shard_model(md, p0, lo, hi, clip) for lo, hi in bounds]
    return EntityShardedTrainer(models=ms), ms


def _whole_run(md, p0, batches, clip):
    m = _whole(md, p0, clip)
    out = []
    for b in batches:
        loss = m.train_step(b).cpu().numpy().copy()
        snap = SC.snapshot([m])
        snap["loss"], snap["norm"] = loss, np.float64(m.train_grad("pred_bias")[1])
        out.append(snap)
    m.close()
    return out


def _sharded_run(md, p0, bounds, batches, clip):
    tr, ms = _trainer(md, p0, bounds, clip)
    out = []
    for b in batches:
        loss = tr.step(b).cpu().numpy().copy()
        SC.replicated_equal(ms)
        snap = SC.snapshot(ms)
        norms = [m.train_grad("pred_bias")[1] for m in ms]
        assert all(n == norms[0] for n in norms), norms      # the global norm, the same double on every rank
        snap["loss"], snap["norm"] = loss, np.float64(norms[0])
        out.append(snap)
    _close(ms)
    return out


def _assert_whole_bits(got, want, clip):
    """Contract 2: everything but the norm's last bits (the whole-table handle adds the table's squares inside one fold)."""
    for step, (g, w) in enumerate(zip(got, want)):
        print("step %d loss %.9g norm %.9g (whole table %.9g)" % (step, float(g["loss"][0]), float(g["norm"]), float(w["norm"])))
        assert 0.0 < float(g["norm"]) < clip and float(w["norm"]) < clip, (g["norm"], w["norm"], clip)      # (the clip factor is exactly 1)
        # (two orders of one sum of n < 1e6 non-negative doubles differ by at most n 2^-53 of it: 1e-10 with room)
        assert abs(float(g["norm"]) - float(w["norm"])) <= 1e-10 * float(w["norm"])
        SC.same_bits({k: v for k, v in g.items() if k != "norm"}, {k: v for k, v in w.items() if k != "norm"}, "step %d" % step)


def _world_of_one(md, batches):
    p0 = _p0(md)
    want = _whole_run(md, p0, batches, SC.CLIP_OFF)
    got = _sharded_run(md, p0, ((0, md["num_ent"]),), batches, SC.CLIP_OFF)
    _assert_whole_bits(got, want, SC.CLIP_OFF)


# ------------------------------------------------------------------------------------------------ contract 2
@pytest.mark.parametrize("name", ["cpg_linear", "plain", "lookup"])
def test_a_world_of_one_is_the_whole_table_handle_bit_for_bit(name):
    """E = 300, B = 48, L = 30, two sampled steps on one shard [0, 300): the fused scorer, one row batch."""
    md = SC.md_for(name, SC.E300)
    _world_of_one(md, [sampled_edge_batch(md, 48, 30, step, _EDGES300) for step in range(2)])


def test_a_world_of_one_with_alternating_label_forms():
    """Sampled, sparse 1-vs-all, sampled: the loss is normalised by the labels of the score call that ran, and neither form leaves
    anything behind for the other."""
    md = SC.md_for("cpg_linear", SC.E300)
    _world_of_one(md, [sampled_edge_batch(md, 48, 30, 0, _EDGES300), SC.batch300(md, 1), sampled_edge_batch(md, 48, 30, 2, _EDGES300)])


def test_a_world_of_one_on_the_scalar_routes():
    """d = 77 and B = 47: k_tr_score_loss, the scalar dh gather and the scalar segment reduce; B d is no multiple of 4."""
    md = SC.md_for("cpg_linear", SC.E300, ent_emb_size=77, emb_h=7, emb_w=11)
    assert (47 * 77) % 4 != 0
    _world_of_one(md, [sampled_edge_batch(md, 47, 30, step, _EDGES300) for step in range(2)])


def test_a_world_of_one_over_three_row_batches():
    """cpg_wide, E = 700, d = 200, L = 150: a row batch of the fused scorer is 60 rows, so a sample walks three, the last one ragged."""
    md = SC.md_for("cpg_wide", 700)
    assert md["ent_emb_size"] == 200
    _world_of_one(md, [sampled_edge_batch(md, 48, 150, step, _EDGES700) for step in range(2)])


def test_a_world_of_one_at_the_fused_route_s_longest_sample():
    """L = 8192 at d = 40: the last L of the fused scorer; its ids and the compacted positions are 64 KiB of LDS beside the row
    batch's 15, so the sharded launch raises the kernel's dynamic-LDS limit (the whole-table launch stays under 64 KiB)."""
    md = SC.md_for("cpg_linear", SC.E300)
    assert md["ent_emb_size"] == 40
    _world_of_one(md, [sampled_edge_batch(md, 6, 8192, step, _EDGES300[:5]) for step in range(2)])


def test_a_world_of_one_past_the_fused_route():
    """L = 8200 > 8192 at d = 40: k_tr_score_loss and the 16-byte dh gather (B = 6 keeps it small)."""
    md = SC.md_for("cpg_linear", SC.E300)
    _world_of_one(md, [sampled_edge_batch(md, 6, 8200, step, _EDGES300[:5]) for step in range(2)])


# ------------------------------------------------------------------------------------------------ contract 3
def _table_grads_case(md, bounds, B, L, edges, min_rows, patch=None):
    p0 = _p0(md)
    E = md["num_ent"]
    batch = sampled_edge_batch(md, B, L, 0, edges)
    if patch is not None:
        patch(batch)
    m = _whole(md, p0, SC.CLIP_OFF)
    m.train_step(batch)
    want = {k: m.train_grad(k)[0].cpu().numpy().copy() for k in SC.TABLES}
    gn = m.train_grad("pred_bias")[1]
    m.close()
    assert gn < SC.CLIP_OFF
    tr, ms = _trainer(md, p0, bounds, SC.CLIP_OFF)
    tr.step(batch)
    got = {k: np.concatenate([m.train_grad(k)[0].cpu().numpy().reshape(hi - lo, -1) for m, (lo, hi) in zip(ms, bounds)]) for k in SC.TABLES}
    _close(ms)
    assert got["pred_bias"].tobytes() == want["pred_bias"].reshape(E, -1).tobytes()
    assert np.count_nonzero(want["pred_bias"]) > 0
    free = np.ones(E, bool)
    free[_clamped(batch, E)["e1"]] = False
    print("rows compared: %d of %d" % (int(free.sum()), E))
    assert int(free.sum()) >= min_rows
    g, w = got["ent_emb"], want["ent_emb"].reshape(E, -1)
    assert g[free].tobytes() == w[free].tobytes()
    assert np.count_nonzero(w[free]) > 0
    return g, w, free


def test_table_gradient_does_not_depend_on_the_sharding_e300():
    md = SC.md_for("cpg_linear", SC.E300)
    _table_grads_case(md, SC.BOUNDS300, 48, 30, _EDGES300, 200)


def test_table_gradient_does_not_depend_on_the_sharding_e700():
    md = SC.md_for("cpg_wide", 700)
    _table_grads_case(md, _BOUNDS700, 48, 150, _EDGES700, 600)


def test_table_gradient_does_not_depend_on_the_sharding_scalar_routes():
    md = SC.md_for("cpg_linear", SC.E300, ent_emb_size=77, emb_h=7, emb_w=11)
    _table_grads_case(md, SC.BOUNDS300, 47, 30, _EDGES300, 200)


def test_table_gradient_does_not_depend_on_the_sharding_three_digit_sort():
    """E = 70,000: three 8-bit digit passes; d = 12: the 16-byte route outside the fused kernel; the bound 33333 sits on no tile and
    no digit edge.  The lookup holds both sides of the bound, the last row, row 0 and 65536 (a carry into the third digit)."""
    md = _small_md(70000)
    ids = (33332, 33333, 69999, 0, 65536)

    def patch(batch):
        batch["lookup_values"][5, :len(ids)] = ids
        assert set(ids) <= set(batch["lookup_values"].ravel().tolist())

    _table_grads_case(md, ((0, 33333), (33333, 70000)), 48, 37, (0, 33332, 33333, 65536, 69999), 200, patch)


# ------------------------------------------------------------------------------------------------ contract 4
def _oracle_step(md, p0, batch, clip):
    from oracle import coper_train_oracle as T
    ref, opt = S.new_oracle(md, p0, clip=clip)
    cb = _clamped(batch, md["num_ent"])
    ob = dict(e1=cb["e1"], rel=cb["rel"], lookup=cb["lookup_values"], labels=cb["e2_multi"])
    return T.train_step(ref, md, ob, opt, seed=SC.SEED, step=0, momentum=md["batch_norm_momentum"])


def test_two_shards_with_the_clip_active_match_the_oracle():
    """cpg_wide, E = 700 as (0,384), (384,700), L = 150, clip_norm below the oracle's norm.  Loss, every leaf's gradient (table rows in
    rank order) and the global norm against the float64 oracle on the clamped batch; a second run from fresh handles leaves identical
    bits."""
    from oracle import coper_train_oracle as T
    md = SC.md_for("cpg_wide", 700)
    p0 = _p0(md)
    batch = sampled_edge_batch(md, 48, 150, 0, _EDGES700)
    loss_o, grads_o, gn_o = _oracle_step(md, p0, batch, SC.CLIP_ACTIVE)
    assert gn_o > 2.0 * SC.CLIP_ACTIVE, gn_o      # the clip acts

    def run():
        tr, ms = _trainer(md, p0, _BOUNDS700, SC.CLIP_ACTIVE)
        loss = float(tr.step(batch).cpu()[0])
        SC.replicated_equal(ms)
        grads, gn = {}, None
        for leaf in T.trainable_names(md):
            parts = [m.train_grad(leaf) for m in (ms if leaf in SC.TABLES else ms[:1])]
            grads[leaf], gn = np.concatenate([g.cpu().numpy() for g, _ in parts]), parts[0][1]
        snap = SC.snapshot(ms)
        snap["loss"], snap["norm"] = np.float32(loss), np.float64(gn)
        _close(ms)
        return loss, grads, gn, snap

    loss, grads, gn, snap = run()
    print("loss %.9g oracle %.9g; norm %.9g oracle %.9g" % (loss, loss_o, gn, gn_o))
    assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (loss, loss_o)
    S.check_grads(grads, grads_o, gn_o, "sharded sampled")
    assert abs(gn - gn_o) < 1e-4 * gn_o, (gn, gn_o)
    SC.same_bits(run()[3], snap, "second run")


def test_a_shard_that_owns_nothing_of_a_batch():
    """E = 300 as BOUNDS300 with every lookup id below 128: shards 1 and 2 hand out exact zeros in dh_part / loss_part, their table
    gradients are zero but for the owned e1 rows, and the step's loss is the oracle's."""
    md = SC.md_for("cpg_linear", SC.E300)
    p0 = _p0(md)
    E, d = SC.E300, md["ent_emb_size"]
    batch = sampled_edge_batch(md, 48, 30, 0, _EDGES300)
    lk = batch["lookup_values"]
    inside = (lk >= 0) & (lk < E)
    batch["lookup_values"] = np.where(inside, lk % 128, lk).astype(np.int32)      # (the four ids outside [0, E) stay: they count as row 0)
    assert _clamped(batch, E)["lookup_values"].max() < 128
    loss_o, _, gn_o = _oracle_step(md, p0, batch, SC.CLIP_OFF)
    assert gn_o < SC.CLIP_OFF

    tr, ms = _trainer(md, p0, SC.BOUNDS300, SC.CLIP_OFF)
    B = len(batch["e1"])
    rows = tr._exchange([m.train_shard_gather(batch["e1"]) for m in ms], reduce=True)
    dh, ls, sq = [], [], []
    for m, r in zip(ms, rows):
        m.train_shard_forward(batch["e1"], batch["rel"], r)
        dh.append(torch.full((B, d), 7.0, device=m.device, dtype=torch.float32))
        ls.append(torch.full((1,), 7.0, device=m.device, dtype=torch.float64))
        sq.append(torch.empty(1, device=m.device, dtype=torch.float64))
        m.train_shard_score_lookup(batch, B, dh[-1], ls[-1])
    assert np.count_nonzero(dh[0].cpu().numpy()) > 0 and float(ls[0][0]) > 0.0
    for g in (1, 2):
        assert not dh[g].cpu().numpy().any() and float(ls[g][0]) == 0.0, g
    dh_all, ls_all = tr._exchange(dh), tr._exchange(ls)
    losses = [m.train_shard_backward(a, l.reshape(-1), s) for m, a, l, s in zip(ms, dh_all, ls_all, sq)]
    loss = float(losses[0].cpu()[0])
    print("loss %.9g oracle %.9g" % (loss, loss_o))
    assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (loss, loss_o)
    e1 = _clamped(batch, E)["e1"]
    for g in (1, 2):
        lo, hi = SC.BOUNDS300[g]
        own = np.zeros(hi - lo, bool)
        own[e1[(e1 >= lo) & (e1 < hi)] - lo] = True
        assert own.any() and not own.all()
        ge = ms[g].train_grad("ent_emb")[0].cpu().numpy().reshape(hi - lo, d)
        assert not ge[~own].any() and np.count_nonzero(ge[own]) > 0, g
        assert not ms[g].train_grad("pred_bias")[0].cpu().numpy().any(), g
    sq_all = tr._exchange(sq)
    for m, s in zip(ms, sq_all):
        m.train_shard_apply(s.reshape(-1))
    SC.replicated_equal(ms)
    _close(ms)


# ------------------------------------------------------------------------------------------------ contract 1 across processes
def _run_ranks(tmp_path, world, **args):
    """Starts `world` ranks of tests/shard_train_sampled_child.py, waits for them under one time limit -> [the .npz of rank r as a dict]"""
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    procs, logs = [], []
    for r in range(world):
        cmd = [sys.executable, os.path.join(ROOT, "tests", "shard_train_sampled_child.py"), "--rank", str(r), "--world", str(world), "--port",
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


def _rank_view(snap, lo, hi):
    """The rows [lo, hi) of the tables in a snapshot of all shards: what rank (lo, hi) alone holds."""
    return {k: (v[lo:hi] if k.split("/")[-1] in SC.TABLES and k.split("/")[0] in ("var", "slot0", "slot1", "slot2") else v) for k, v in snap.items()}


def test_two_processes_leave_the_bits_of_the_in_process_form(tmp_path):
    """E = 300 as (0,150), (150,300) in two processes (RCCL on two GPUs, else gloo on one) and as two handles of one process, two
    sampled steps with the clip active: every rank's file equals the in-process form's bits, step by step."""
    md = SC.md_for("cpg_linear", SC.E300)
    bounds = ((0, 150), (150, 300))
    ranks = _run_ranks(tmp_path, 2, case="cpg_linear", num_ent=SC.E300, bounds=bounds, edges=_EDGES300, batch=48, labels=30, steps=2,
                       clip=SC.CLIP_ACTIVE)
    got = _sharded_run(md, _p0(md), bounds, [sampled_edge_batch(md, 48, 30, step, _EDGES300) for step in range(2)], SC.CLIP_ACTIVE)
    for r, (lo, hi) in enumerate(bounds):
        for step in range(2):
            mine = {k[len("s%d/" % step):]: v for k, v in ranks[r].items() if k.startswith("s%d/" % step)}
            assert float(mine["norm"]) > 2.0 * SC.CLIP_ACTIVE      # (the clip acts: the gathered norm matters to every bit compared here)
            SC.same_bits(mine, _rank_view(got[step], lo, hi), "rank %d step %d" % (r, step))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_call_order():
    """The new call's place in the state machine and its argument checks, by status and by a word of the message; the trainer's
    refusal of dense labels."""
    EINVAL, ESTATE = 1, 5
    md = SC.md_for("cpg_linear", SC.E300)
    p0 = _p0(md)
    m = SC.shard_model(md, p0, 128, 256, SC.CLIP_OFF)
    lib, h = m._lib, m._h

    def refused(rc, code, *words):
        assert rc == code, (rc, code, lib.coper_last_error(h))
        for word in words:
            assert word.encode() in lib.coper_last_error(h), (word, lib.coper_last_error(h))

    b = sampled_edge_batch(md, 48, 30, 0, _EDGES300)
    c = SC.batch300(md, 0)
    B, L, d = 48, 30, md["ent_emb_size"]
    dev = m.device
    e1, rel = m._ids(b["e1"]), m._ids(b["rel"])
    lk = m._ids(b["lookup_values"], torch.int32)
    lab = torch.as_tensor(b["e2_multi"]).to(dev)
    ip, ix, row = m._ids(c["lab_indptr"]), m._ids(c["lab_idx"]), m._ids(c["lab_row"])
    rows = torch.zeros((B, d), device=dev)
    dh, ls, sq = torch.zeros((1, B, d), device=dev), torch.zeros(1, device=dev, dtype=torch.float64), torch.zeros(1, device=dev, dtype=torch.float64)
    loss = torch.zeros(1, device=dev)
    P, st = lambda t: C.c_void_p(t.data_ptr()), m._stream()
    fwd = lambda: lib.coper_train_shard_forward(h, P(e1), P(rel), P(rows), B, None, st)
    score = lambda: lib.coper_train_shard_score_lookup(h, P(lk), P(lab), B, L, P(dh), P(ls), st)
    score_csr = lambda: lib.coper_train_shard_score_csr(h, P(ip), P(ix), P(row), ip.numel() - 1, B, P(dh), P(ls), st)
    bwd = lambda: lib.coper_train_shard_backward(h, P(dh), P(ls), 1, P(loss), P(sq), st)
    app = lambda: lib.coper_train_shard_apply(h, P(sq), 1, st)

    refused(score(), ESTATE, "coper_train_shard_forward")                  # before the forward call
    assert fwd() == 0
    refused(fwd(), ESTATE, "coper_train_shard_score_csr", "coper_train_shard_score_lookup")      # either score call is next
    refused(lib.coper_train_shard_score_lookup(h, None, P(lab), B, L, P(dh), P(ls), st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_score_lookup(h, P(lk), None, B, L, P(dh), P(ls), st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_score_lookup(h, P(lk), P(lab), B, L, None, P(ls), st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_score_lookup(h, P(lk), P(lab), B, L, P(dh), None, st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_score_lookup(h, P(lk), P(lab), B, 0, P(dh), P(ls), st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_score_lookup(h, P(lk), P(lab), B - 1, L, P(dh), P(ls), st), EINVAL, "forward call")
    assert score() == 0
    refused(score(), ESTATE, "coper_train_shard_backward")                 # twice in a row
    assert bwd() == 0 and app() == 0
    assert fwd() == 0 and score_csr() == 0
    refused(score(), ESTATE, "coper_train_shard_backward")                 # after the other score call
    assert bwd() == 0 and app() == 0
    torch.cuda.synchronize()
    m.close()

    # a state that is not entity-sharded
    from coper_amd.models import ConvE
    w = ConvE(md, device="cuda:0")
    w.load_parameters({k: torch.as_tensor(v) for k, v in SC.host_params(p0).items()})
    lib, h = w._lib, w._h
    refused(lib.coper_train_shard_score_lookup(h, P(lk), P(lab), B, L, P(dh), P(ls), w._stream()), ESTATE, "coper_train_init_sharded")
    w.train_init(seed=SC.SEED, deterministic=True, ordered_rows=True)
    refused(lib.coper_train_shard_score_lookup(h, P(lk), P(lab), B, L, P(dh), P(ls), w._stream()), ESTATE, "not an entity-sharded state")
    w.close()

    # the trainer: a dense [B, num_ent] e2_multi is still refused; a sampled batch whose arrays disagree never reaches the library
    tr, ms = _trainer(md, p0, ((0, SC.E300),), SC.CLIP_OFF)
    dense = dict(e1=b["e1"], rel=b["rel"], e2_multi=np.zeros((B, SC.E300), np.float32), lookup_values=np.zeros((B, 0), np.int32))
    with pytest.raises(ValueError, match="dense e2_multi"):
        tr.step(dense)
    with pytest.raises(ValueError, match="dense e2_multi"):
        tr.step(dict(e1=b["e1"], rel=b["rel"], e2_multi=dense["e2_multi"]))
    _close(ms)
