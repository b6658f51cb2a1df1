"""GPU tests of entity-sharded 1-vs-all training (include/coper_hip.h "Entity-sharded training"; coper_amd.parallel.EntityShardedTrainer;
DESIGN.md 6.7).

What the bits must be: where every shard is exactly one chunk of one_vs_all_chunk columns (the last one ragged) and the global norm is
below clip_norm, a sharded step leaves the bits of `train_init(deterministic=True, one_vs_all_chunk=w)` + `train_step` on a whole-table
handle -- loss, variables, slots, BN statistics.  Where a shard walks several chunks or the clip acts, only the association of a sum
differs: those runs are held to the float64 oracle by the bounds of tests/test_gpu_train_csr.py::_check_against_oracle (loss
2e-5 max(1, |loss|); gradients 2e-4 by _rel_err; norm 1e-4 relative).  Across runs, handles, processes and the two trainer forms the
bits are always the same.

Ranks in processes of their own (tests/shard_train_child.py) are started as tests/test_gpu_train_parallel.py starts its ranks: one time
limit per run, the first bad exit status ends it, nothing is started again."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIMIT = 150.0      # seconds for the ranks of one run (init_process_group itself gives up after 60)
_EDGES300 = (0, 127, 128, 255, 256, 299)


def _p0(md):
    return cdata.synthetic_params(md, seed=21, ent_std=0.1)


def _trainer(md, p0, bounds, clip, chunk=SC.CHUNK, score_mode="f32"):
    from coper_amd.parallel import EntityShardedTrainer
    ms = [SC.shard_model(md, p0, lo, hi, clip, chunk=chunk, score_mode=score_mode) for lo, hi in bounds]
    return EntityShardedTrainer(models=ms), ms


def _close(ms):
    for m in ms:
        m.close()


def _single_run(md, p0, batches, clip, chunk=SC.CHUNK):
    """The whole-table deterministic handle over `batches` -> ([snapshot + loss + norm per step], the model)"""
    m = SC.single_model(md, p0, clip, chunk=chunk)
    out = []
    for b in batches:
        loss = m.train_step(b).cpu().numpy().copy()
        snap = SC.snapshot([m])
        snap["loss"], snap["norm"] = loss, np.float64(m.train_grad("pred_bias")[1])
        out.append(snap)
    return out, m


def _sharded_run(md, p0, bounds, batches, clip, chunk=SC.CHUNK, score_mode="f32"):
    tr, ms = _trainer(md, p0, bounds, clip, chunk, score_mode)
    out = []
    for b in batches:
        loss = tr.step(b).cpu().numpy().copy()
        SC.replicated_equal(ms)
        snap = SC.snapshot(ms)
        norms = [m.train_grad("pred_bias")[1] for m in ms]
        assert all(n == norms[0] for n in norms), norms      # the global norm, the same double on every rank
        snap["loss"], snap["norm"] = loss, np.float64(norms[0])
        out.append(snap)
    return out, ms


def _assert_single_bits(got, want, clip):
    """Case 1's contract: everything but the norm's last bits (the single handle adds the table's squares inside one fold)."""
    for step, (g, w) in enumerate(zip(got, want)):
        print("step %d loss %.9g norm %.9g (single handle %.9g)" % (step, float(g["loss"][0]), float(g["norm"]), float(w["norm"])))
        assert 0.0 < float(g["norm"]) < clip and float(w["norm"]) < clip, (g["norm"], w["norm"], clip)      # (the clip factor is exactly 1)
        # (two orders of one sum of n < 1e6 non-negative doubles differ by at most n 2^-53 of it: 1e-10 with room)
        assert abs(float(g["norm"]) - float(w["norm"])) <= 1e-10 * float(w["norm"])
        SC.same_bits({k: v for k, v in g.items() if k != "norm"}, {k: v for k, v in w.items() if k != "norm"}, "step %d" % step)


@pytest.mark.parametrize("name", ["cpg_linear", "plain", "lookup"])
def test_one_chunk_per_shard_is_the_single_handle_bit_for_bit(name):
    """E = 300 at chunk 128 as shards (0,128), (128,256), (256,300); B = 48, two steps; labels on both sides of every bound, at the
    first and the last column, an empty row; e1 on both sides of every bound and one id twice.  The same with one shard that is the
    whole table (a world of one: three chunks in one call)."""
    md = SC.md_for(name, SC.E300)
    p0 = _p0(md)
    batches = [SC.batch300(md, step) for step in range(2)]
    e1 = batches[0]["e1"]
    assert {127, 128, 255, 256} <= set(e1.tolist()) and len(set(e1.tolist())) < len(e1)
    want, m = _single_run(md, p0, batches, SC.CLIP_OFF)
    m.close()
    got, ms = _sharded_run(md, p0, SC.BOUNDS300, batches, SC.CLIP_OFF)
    _close(ms)
    _assert_single_bits(got, want, SC.CLIP_OFF)
    got1, ms = _sharded_run(md, p0, ((0, SC.E300),), batches, SC.CLIP_OFF)
    _close(ms)
    _assert_single_bits(got1, want, SC.CLIP_OFF)


def test_scalar_routes_are_the_single_handle_bit_for_bit():
    """d = 77 and B = 47: B d and d are no multiples of 4, so the fold of the dh shares and the owned-row add take their scalar routes
    (every table still 16-byte aligned, as the deterministic mode asks).  Case 1's contract."""
    md = SC.md_for("cpg_linear", SC.E300, ent_emb_size=77, emb_h=7, emb_w=11)
    p0 = _p0(md)
    batches = [SC.batch300(md, step, B=47) for step in range(2)]
    assert (47 * 77) % 4 != 0
    want, m = _single_run(md, p0, batches, SC.CLIP_OFF)
    m.close()
    got, ms = _sharded_run(md, p0, SC.BOUNDS300, batches, SC.CLIP_OFF)
    _close(ms)
    _assert_single_bits(got, want, SC.CLIP_OFF)


def test_several_chunks_per_shard_with_the_clip_active_match_the_oracle():
    """E = 700, d = 200, chunk 128, shards (0,384) and (384,700): three chunks each, the second one's last ragged.  clip_norm below
    the oracle's norm.  Loss, every leaf's gradient (table rows in rank order) and the global norm against the float64 oracle; the
    replicated leaves and slots byte-equal on both handles; a second run from fresh handles leaves identical bits."""
    from oracle import coper_train_oracle as T
    md = SC.md_for("cpg_wide", 700)
    p0 = _p0(md)
    bounds = ((0, 384), (384, 700))
    batch = SC.edge_batch(md, 48, 0, (0, 127, 128, 383, 384, 699))
    ref, opt = S.new_oracle(md, p0, clip=SC.CLIP_ACTIVE)
    loss_o, grads_o, gn_o = T.train_step(ref, md, S.oracle_batch(md, batch), opt, seed=SC.SEED, step=0, momentum=md["batch_norm_momentum"])
    assert gn_o > 2.0 * SC.CLIP_ACTIVE, gn_o      # the clip acts

    def run():
        tr, ms = _trainer(md, p0, bounds, SC.CLIP_ACTIVE)
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
    S.check_grads(grads, grads_o, gn_o, "sharded")
    assert abs(gn - gn_o) < 1e-4 * gn_o, (gn, gn_o)
    SC.same_bits(run()[3], snap, "second run")


def _run_ranks(tmp_path, world, **args):
    """Starts `world` ranks of tests/shard_train_child.py, waits for them under one time limit -> [the .npz of rank r as a dict]"""
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    procs, logs = [], []
    for r in range(world):
        cmd = [sys.executable, os.path.join(ROOT, "tests", "shard_train_child.py"), "--rank", str(r), "--world", str(world), "--port", str(port),
               "--backend", backend, "--out", str(tmp_path / ("rank%d.npz" % r))]
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
    """E = 300 as (0,150), (150,300) -- two chunks per shard -- in two processes (RCCL on two GPUs, else gloo on one) and as two handles
    of one process: every rank's file equals the in-process form's bits, step by step."""
    md = SC.md_for("cpg_linear", SC.E300)
    bounds = ((0, 150), (150, 300))
    ranks = _run_ranks(tmp_path, 2, case="cpg_linear", num_ent=SC.E300, bounds=bounds, edges=_EDGES300, steps=2, clip=SC.CLIP_ACTIVE)
    got, ms = _sharded_run(md, _p0(md), bounds, [SC.edge_batch(md, 48, step, _EDGES300) for step in range(2)], SC.CLIP_ACTIVE)
    _close(ms)
    for r, (lo, hi) in enumerate(bounds):
        for step in range(2):
            mine = {k[len("s%d/" % step):]: v for k, v in ranks[r].items() if k.startswith("s%d/" % step)}
            assert float(mine["norm"]) > SC.CLIP_ACTIVE      # (the clip acts: the gathered norm matters to every bit compared here)
            SC.same_bits(mine, _rank_view(got[step], lo, hi), "rank %d step %d" % (r, step))


@pytest.mark.parametrize("score_mode", ["f32", "bf16x3"])
def test_train_sharded_then_rank_sharded(tmp_path, score_mode):
    """E = 256 as (0,128), (128,256) at chunk 128: two sharded steps in two processes, then prepare() on the shards and
    EntityShardedRanker over them.  The ranks are those of the whole-table handle trained by the same two steps."""
    E = 256
    md = SC.md_for("cpg_linear", E)
    edges = (0, 127, 128, 255)
    bounds = ((0, 128), (128, 256))
    ranks = _run_ranks(tmp_path, 2, case="cpg_linear", num_ent=E, bounds=bounds, edges=edges, steps=2, clip=SC.CLIP_OFF, score_mode=score_mode,
                       rank_queries=96)
    from coper_amd.models import ConvE
    p0 = _p0(md)
    m = ConvE(md, device="cuda:0", score_mode=score_mode)
    m.load_parameters({k: torch.as_tensor(v) for k, v in SC.host_params(p0).items()})
    m.train_init(seed=SC.SEED, clip_norm=SC.CLIP_OFF, deterministic=True, one_vs_all_chunk=SC.CHUNK)
    for step in range(2):
        m.train_step(SC.edge_batch(md, 48, step, edges))
    for r, (lo, hi) in enumerate(bounds):      # (one chunk per shard, no clip: the trained tables are the single handle's rows)
        assert ranks[r]["s1/var/ent_emb"].tobytes() == m._tensors["ent_emb"][lo:hi].cpu().numpy().tobytes()
    q = cdata.synthetic_queries(md, 96, seed=3)
    m.prepare()
    want, want_ne = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
    for r in range(2):
        assert np.array_equal(ranks[r]["ranks"], want.cpu().numpy()), r
        assert np.array_equal(ranks[r]["n_equal"], want_ne.cpu().numpy()), r
    m.close()


def test_sharded_state_holds_the_own_rows_only():
    """E = 20,000, d = 200, a shard of E / 4: the training state (coper_live_device_bytes around the init call) is smaller than the
    whole-table state by the gradient and the three slots of the absent rows, 4 * 4 * (E - n_local) * (d + 1) bytes -- less at most
    the pad that rounds the smaller state up to a 4 KiB allocation granule."""
    from coper_amd import _lib
    from coper_amd.models import ConvE
    lib = _lib.load()
    md = SC.md_for("cpg_wide", 20000)
    E, d, n_local = 20000, md["ent_emb_size"], 5000
    p0 = SC.host_params(_p0(md))

    def state_bytes(shard, sharded):
        m = ConvE(md, device="cuda:0", shard=shard)
        m.load_parameters({k: torch.as_tensor(v) for k, v in p0.items()})
        before = lib.coper_live_device_bytes()
        m.train_init(seed=SC.SEED, deterministic=True, entity_sharded=sharded, one_vs_all_chunk=SC.CHUNK)
        grew = lib.coper_live_device_bytes() - before
        n = C.c_int64()
        _lib.check(m._h, lib.coper_train_slot(m._h, b"ent_emb", 0, None, 0, 0, C.byref(n), None))
        m.close()
        return grew, n.value

    whole, n_whole = state_bytes(None, False)
    part, n_part = state_bytes((E // 2, E // 2 + n_local), True)
    assert (n_whole, n_part) == (E * d, n_local * d)
    granule = (-part) % 4096
    print("training state: whole table %d bytes, a quarter shard %d bytes" % (whole, part))
    assert whole - part >= 4 * 4 * (E - n_local) * (d + 1) - granule, (whole, part, granule)


def test_refusals_and_call_order():
    """Every refusal of the header section, by status and by a word of the message: the state machine's order, the calls a sharded
    state does not serve, coper_train_init on a shard handle (unchanged), the default mode, bad arguments."""
    from coper_amd import _lib
    from coper_amd._lib import CoperError
    EINVAL, ESTATE, EUNSUPPORTED = 1, 5, 7
    md = SC.md_for("cpg_linear", SC.E300)
    p0 = _p0(md)
    lo, hi = 128, 256
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0", shard=(lo, hi))
    m.load_parameters({k: torch.as_tensor(v) for k, v in SC.host_params(p0).items()})
    lib, h = m._lib, m._h

    def refused(rc, code, word):
        assert rc == code, (rc, code, lib.coper_last_error(h))
        assert word.encode() in lib.coper_last_error(h), (word, lib.coper_last_error(h))

    with pytest.raises(CoperError, match="whole entity table"):      # the existing init keeps its refusal and its text
        m.train_init(seed=SC.SEED, deterministic=True)
    with pytest.raises(CoperError, match="deterministic") as ei:     # the default mode is not built
        m.train_init(seed=SC.SEED, deterministic=False, entity_sharded=True)
    assert ei.value.code == EUNSUPPORTED
    assert lib.coper_train_sharded(h) == -ESTATE
    m.train_init(seed=SC.SEED, clip_norm=SC.CLIP_OFF, deterministic=True, entity_sharded=True, one_vs_all_chunk=SC.CHUNK)
    assert m.train_sharded == 1 and m.train_deterministic == 1

    b = SC.batch300(md, 0)
    B, d = len(b["e1"]), md["ent_emb_size"]
    dev = m.device
    e1, rel = m._ids(b["e1"]), m._ids(b["rel"])
    ip, ix, row = m._ids(b["lab_indptr"]), m._ids(b["lab_idx"]), m._ids(b["lab_row"])
    rows = torch.zeros((B, d), device=dev)
    dh, ls, sq = torch.zeros((1, B, d), device=dev), torch.zeros(1, device=dev, dtype=torch.float64), torch.zeros(1, device=dev, dtype=torch.float64)
    loss = torch.zeros(1, device=dev)
    P, st = lambda t: C.c_void_p(t.data_ptr()), m._stream()
    fwd = lambda: lib.coper_train_shard_forward(h, P(e1), P(rel), P(rows), B, None, st)
    score = lambda: lib.coper_train_shard_score_csr(h, P(ip), P(ix), P(row), ip.numel() - 1, B, P(dh), P(ls), st)
    bwd = lambda: lib.coper_train_shard_backward(h, P(dh), P(ls), 1, P(loss), P(sq), st)
    app = lambda: lib.coper_train_shard_apply(h, P(sq), 1, st)

    # out of order: the text names the call expected next
    refused(score(), ESTATE, "coper_train_shard_forward")
    refused(bwd(), ESTATE, "coper_train_shard_forward")
    refused(app(), ESTATE, "coper_train_shard_forward")
    # bad arguments in their phase
    refused(lib.coper_train_shard_forward(h, P(e1), P(rel), None, B, None, st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_forward(h, P(e1), P(rel), P(rows), 0, None, st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_gather(h, None, B, P(rows), st), EINVAL, "bad argument")
    assert fwd() == 0
    refused(fwd(), ESTATE, "coper_train_shard_score_csr")
    refused(app(), ESTATE, "coper_train_shard_score_csr")
    refused(lib.coper_train_shard_score_csr(h, P(ip), P(ix), P(row), ip.numel() - 1, B, None, P(ls), st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_score_csr(h, P(ip), P(ix), P(row), ip.numel() - 1, B - 1, P(dh), P(ls), st), EINVAL, "forward call")
    assert score() == 0
    refused(score(), ESTATE, "coper_train_shard_backward")
    refused(lib.coper_train_shard_backward(h, P(dh), P(ls), 0, P(loss), P(sq), st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_backward(h, None, P(ls), 1, P(loss), P(sq), st), EINVAL, "bad argument")
    assert bwd() == 0
    refused(fwd(), ESTATE, "coper_train_shard_apply")
    refused(lib.coper_train_shard_apply(h, P(sq), 0, st), EINVAL, "bad argument")
    refused(lib.coper_train_shard_apply(h, None, 1, st), EINVAL, "bad argument")
    assert app() == 0
    refused(app(), ESTATE, "coper_train_shard_forward")
    torch.cuda.synchronize()

    # what a sharded state does not serve
    lab = torch.zeros((B, 4), device=dev)
    lk = torch.zeros((B, 4), device=dev, dtype=torch.int32)
    a9 = (h, P(e1), P(rel), P(lk), P(lab), B, 4, P(loss), st)
    a10 = (h, P(e1), P(rel), P(ip), P(ix), P(row), ip.numel() - 1, B, P(loss), st)
    refused(lib.coper_train_step(*a9), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_backward(*a9), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_forward(h, P(e1), P(rel), P(lk), P(lab), B, 4, P(loss), None, None, st), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_step_csr(*a10), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_backward_csr(*a10), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_forward_csr(h, P(e1), P(rel), P(ip), P(ix), P(row), ip.numel() - 1, B, P(loss), None, None, st), EUNSUPPORTED,
            "entity-sharded")
    flat = torch.zeros(64, device=dev)
    refused(lib.coper_train_grads_export(h, P(flat), 64, 0, st), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_apply(h, P(flat), 64, 1.0, st), EUNSUPPORTED, "coper_train_shard_apply")
    refused(lib.coper_train_defer_rows(h, 1, st), EUNSUPPORTED, "entity-sharded")
    refused(lib.coper_train_order_rows(h, 1, st), EUNSUPPORTED, "entity-sharded")
    # the tables' gradient and slots are the local rows; the norm is a finite global one
    g, gn = m.train_grad("ent_emb")
    assert g.numel() == (hi - lo) * d and np.isfinite(gn) and gn > 0.0
    slots, _ = m.optimizer_state()
    assert slots["ent_emb"][0].shape == (hi - lo, d) and slots["pred_bias"][2].shape == (hi - lo,)
    m.close()

    # the trainer's construction checks
    from coper_amd.parallel import EntityShardedTrainer
    ms = [SC.shard_model(md, p0, 0, 128, SC.CLIP_OFF), SC.shard_model(md, p0, 128, 256, SC.CLIP_OFF)]
    with pytest.raises(ValueError, match="end at"):
        EntityShardedTrainer(models=ms)
    with pytest.raises(ValueError, match="rank order"):
        EntityShardedTrainer(models=ms[::-1])
    ms.append(SC.shard_model(md, p0, 256, 300, 2.0 * SC.CLIP_OFF))
    with pytest.raises(ValueError, match="hyper-parameters"):
        EntityShardedTrainer(models=ms)
    _close(ms)
