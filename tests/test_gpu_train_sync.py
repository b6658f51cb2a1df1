"""GPU tests of the backward whose batch statistics span all ranks (include/coper_hip.h, "Synchronised batch statistics: the backward in
phases"): coper_train_sync_begin | _csr, coper_train_sync_next.  The G replicas are G handles in one process, the
all-gather between two calls is torch.stack in rank order.  Shapes are tests/test_gpu_train.py::_CASES, batches and the float64 oracle
those of tests/split_common.py; the whole batch is B_global = 48 samples with L = 16 labels each.  Every test here fails on a library
without the calls."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from coper_amd._lib import CoperError
from coper_amd.models import _ptr
from coper_amd.parallel import shard_batch
from tests import split_common as S
from tests import train_history_common as TH
from tests.test_gpu_train import _rel_err
from tests.test_gpu_train_deterministic import _assert_same_bits, _outputs

pytestmark = pytest.mark.gpu

BG, L, BATCH_SEED = 48, 16, 7
EINVAL, ESTATE, EUNSUPPORTED = 1, 5, 7
BOUND = 2e-4      # S.check_grads: the project's bound on _rel_err


def _p0(md):
    return cdata.synthetic_params(md, seed=21, ent_std=0.1)


def _model(md, p0, deterministic, **kw):
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=S.SEED, clip_norm=S.CLIP, deterministic=deterministic, **kw)
    return m


def _sync_backward(ms, shards, rows=False, stop_at=None):
    """The phase loop over the replicas `ms` (rank = position): begin on every replica, then next with the parts stacked in rank order
    until a call hands out nothing -> ([loss of rank r], [n of every exchange]).  stop_at: leave the step open in front of that exchange."""
    G = len(ms)
    B = len(shards[0]["e1"])
    outs = [m.train_sync_begin(sh, G * B, r * B, rows=rows) for r, (m, sh) in enumerate(zip(ms, shards))]
    ns = []
    while outs[0][1]:
        n = outs[0][1]
        assert all(o[1] == n for o in outs)
        ns.append(n)
        assert all(m.train_sync_phase == len(ns) for m in ms)
        if stop_at == len(ns):
            return None, ns
        parts = torch.stack([p[:n] for p, _ in outs])      # the all-gather: [G, n] in rank order
        outs = [m.train_sync_next(parts) for m in ms]
    assert all(m.train_sync_phase == 0 for m in ms)
    return [m.train_sync_loss.clone() for m in ms], ns


def _part_lens(md):
    C_, d = md["conv_num_channels"], md["ent_emb_size"]
    return [2 * C_, 2 * d, 2 * d, 2 * C_]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name,form", [("cpg_linear", "sampled"), ("plain", "dense"), ("cpg_linear", "csr")])
def test_world_of_one_is_train_backward_bit_for_bit(name, form):
    """Deterministic mode: begin + four next, each handed this handle's own part, against train_backward on a twin: the loss, the flat
    gradient and the moving statistics byte for byte; after train_apply every variable and slot."""
    md = S.md_for(name)
    p0 = _p0(md)
    a, b = _model(md, p0, True), _model(md, p0, True)
    batch = S.batch(md, form, BG, L, BATCH_SEED)
    (loss_a,), ns = _sync_backward([a], [batch])
    assert ns == _part_lens(md)
    loss_b = b.train_backward(batch)
    assert loss_a.cpu().numpy().tobytes() == loss_b.cpu().numpy().tobytes()
    assert a.train_grads_export().cpu().numpy().tobytes() == b.train_grads_export().cpu().numpy().tobytes()
    for k in a._tensors:
        if k.endswith(("moving_mean", "moving_variance")):
            assert a._tensors[k].cpu().numpy().tobytes() == b._tensors[k].cpu().numpy().tobytes(), k
    a.train_apply()
    b.train_apply()
    _assert_same_bits(_outputs(a, loss_a), _outputs(b, loss_b), "%s %s: the phased step against train_backward" % (name, form))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2
@functools.lru_cache(maxsize=None)
def _oracle(name, form):
    """ONE float64 step on the whole batch (computed once per case and label form, shared by every world size and mode; read only)."""
    md = S.md_for(name)
    p0 = _p0(md)
    batch = S.batch(md, form, BG, L, BATCH_SEED)
    ref, opt = S.new_oracle(md, p0)
    loss_o, grads_o = S.oracle_backward(ref, md, batch, S.SEED, 0)
    _, gn_o = S.oracle_update(ref, opt, [grads_o])
    return md, p0, batch, loss_o, grads_o, gn_o, ref


_GRAD_CASES = [(n, "sampled") for n in ("cpg_linear", "plain", "cpg_linear_concat", "lookup", "cpg_conv_fc", "cpg_mlp2", "cpg_linear_c32",
                                         "cpg_wide")]
_GRAD_CASES += [(n, f) for n in ("cpg_linear", "plain") for f in ("dense", "csr")]


@pytest.mark.parametrize("deterministic", [True, False], ids=["det", "default"])
@pytest.mark.parametrize("G", [2, 3, 4])
@pytest.mark.parametrize("name,form", _GRAD_CASES)
def test_ranks_make_one_step_on_the_whole_batch(name, form, G, deterministic):
    """G replicas on even shards, dropout on (0.3 / 0.2): the sum of their flat gradients / G against the oracle's gradient of the WHOLE
    batch by S.check_grads, and after train_apply(flat, 1 / G) every variable AND moving statistic by S.check_variables.  The
    unsynchronised route on the same shards -- train_backward per shard, the gradients averaged -- must exceed the bound: the inputs
    tell the two apart.  Deterministic mode: the replicas end byte-identical."""
    md, p0, batch, loss_o, grads_o, gn_o, ref = _oracle(name, form)
    shards = [shard_batch(batch, r, G) for r in range(G)]
    floor = 1e-3 * gn_o

    ms = [_model(md, p0, deterministic) for _ in range(G)]
    layout = ms[0].train_grads_layout()[0]
    flat = None
    for m, sh in zip(ms, shards):
        m.train_backward(sh)
        flat = m.train_grads_export(flat, accumulate=flat is not None)
    unsynced = S.flat_slices(flat.cpu().numpy() * np.float32(1.0 / G), layout)
    worst = max(_rel_err(unsynced[leaf].reshape(w.shape), w, floor) for leaf, w in grads_o.items())
    print("unsynchronised: worst rel err %.3g" % worst)
    assert worst > BOUND, worst
    for m in ms:
        m.close()

    ms = [_model(md, p0, deterministic) for _ in range(G)]
    losses, ns = _sync_backward(ms, shards)
    assert ns == _part_lens(md)
    loss = float(np.mean([float(x.cpu()[0]) for x in losses]))      # (even shards: the mean of the shard means)
    print("loss %.9g oracle %.9g" % (loss, loss_o))
    assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o))
    flat = None
    for m in ms:      # the all-reduce: rank order
        flat = m.train_grads_export(flat, accumulate=flat is not None)
    got = S.flat_slices(flat.cpu().numpy() * np.float32(1.0 / G), layout)
    dg = S.check_grads(got, grads_o, gn_o, "G = %d" % G)
    for m in ms:
        m.train_apply(flat, 1.0 / G)
    gn = ms[0].train_grad("ent_emb")[1]
    assert abs(gn - gn_o) < 1e-4 * gn_o, (gn, gn_o)
    S.check_variables(md, {k: v.cpu().numpy() for k, v in ms[0]._tensors.items()}, ref, dg, "G = %d" % G, skip_stats=False)
    if deterministic:
        first = _outputs(ms[0], losses[0])
        for r in range(1, G):
            other = _outputs(ms[r], losses[0])
            for k in first:      # (every replica keeps its OWN shard's gradients and loss; what an update leaves is equal)
                if k.startswith(("var/", "slot", "power/")) or k == "global_norm":
                    assert np.asarray(first[k]).tobytes() == np.asarray(other[k]).tobytes(), (r, k)
    for m in ms:
        m.close()


# ------------------------------------------------------------------------------------------------ 3
def test_rows_route():
    """The deferred-rows mode (deterministic, ordered rows), G = 2, rows=True: export / import / apply as DataParallelTrainer._step_rows
    makes them.  The replicas end byte-identical; after train_sync_rows the variables are within check_variables of the whole-batch oracle."""
    md, p0, batch, loss_o, grads_o, gn_o, ref = _oracle("cpg_linear", "sampled")
    G = 2
    shards = [shard_batch(batch, r, G) for r in range(G)]
    ms = [_model(md, p0, True, ordered_rows=True, deferred_rows=True) for _ in range(G)]
    losses, ns = _sync_backward(ms, shards, rows=True)
    assert ns == _part_lens(md)
    exported = [m.train_rows_export() for m in ms]
    small = exported[0][0] + exported[1][0]      # the all-reduce
    for m in ms:
        for r in range(G):      # every rank imports every block, its own included, in rank order
            m.train_rows_import(exported[r][1], exported[r][2], first=r == 0)
    layout = ms[0].train_rows_layout()[0]
    a = small.cpu().numpy() * np.float32(1.0 / G)
    got = {leaf: a[off:off + n] for leaf, (off, n) in layout.items()}
    for leaf in ("ent_emb", "pred_bias"):
        got[leaf] = ms[0].train_grad(leaf)[0].cpu().numpy() * np.float32(1.0 / G)
    dg = S.check_grads(got, grads_o, gn_o, "rows")
    for m in ms:
        m.train_rows_apply(small, 1.0 / G)
        m.train_sync_rows()
    S.check_variables(md, {k: v.cpu().numpy() for k, v in ms[0]._tensors.items()}, ref, dg, "rows", skip_stats=False)
    s0, s1 = TH.state_bits(ms[0]), TH.state_bits(ms[1])
    _assert_same_bits(s0, s1, "rank 0 against rank 1")
    for m in ms:
        m.close()


# ------------------------------------------------------------------------------------------------ 4
def test_statistics_off_is_one_call():
    """batch_norm_train_stats = False: nothing to exchange -- begin runs the whole backward, hands out nothing and leaves
    train_backward's bytes (deterministic)."""
    md = S.md_for("cpg_linear", batch_norm_train_stats=False)
    p0 = _p0(md)
    a, b = _model(md, p0, True), _model(md, p0, True)
    batch = S.batch(md, "sampled", BG, L, BATCH_SEED)
    shard = shard_batch(batch, 0, 2)
    part, n = a.train_sync_begin(shard, BG // 2, 0)      # (its own batch: with an offset the masks would be another batch's)
    assert n == 0 and a.train_sync_phase == 0
    loss_a, loss_b = a.train_sync_loss.clone(), b.train_backward(shard)
    assert a.train_grads_export().cpu().numpy().tobytes() == b.train_grads_export().cpu().numpy().tobytes()
    a.train_apply()
    b.train_apply()
    _assert_same_bits(_outputs(a, loss_a), _outputs(b, loss_b), "statistics off")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5
def _code(call):
    with pytest.raises(CoperError) as bad:
        call()
    return bad.value.code


@pytest.mark.parametrize("name", ["cpg_mlp_bn", "cpg_conv_mlp", "cpg_conv_static_fc"])
def test_hidden_generator_bn_is_refused(name):
    md = S.md_for(name)
    m = _model(md, _p0(md), True)
    shard = shard_batch(S.batch(md, "sampled", BG, L, BATCH_SEED), 0, 2)
    assert _code(lambda: m.train_sync_begin(shard, BG, 0)) == EUNSUPPORTED
    assert m.train_sync_phase == 0
    m.train_backward(shard)      # (the handle stays usable)
    m.close()


def test_refusals():
    md = S.md_for("cpg_linear")
    p0 = _p0(md)
    m = _model(md, p0, True)
    lib, h = m._lib, m._h
    shard = shard_batch(S.batch(md, "sampled", BG, L, BATCH_SEED), 1, 2)
    B = BG // 2
    e1, rel, lookup = m._ids(shard["e1"]), m._ids(shard["rel"]), m._ids(shard["lookup_values"], torch.int32)
    labels = torch.as_tensor(shard["e2_multi"]).to("cuda:0").contiguous()
    cap = int(lib.coper_train_sync_part_len(h))
    assert cap == 2 * max(md["conv_num_channels"], md["ent_emb_size"])
    part = torch.zeros(cap + 1, device="cuda:0", dtype=torch.float64)
    odd = C.c_void_p(part.data_ptr() + 4)      # (4 bytes past a double)
    n = C.c_int64(-1)

    def begin(B_global=BG, off=B, rows=0, part_out=_ptr(part), part_cap=cap, n_out=C.byref(n)):
        return lib.coper_train_sync_begin(h, _ptr(e1), _ptr(rel), _ptr(lookup), _ptr(labels), B, L, B_global, off, rows, part_out, part_cap, n_out,
                                          _ptr(m._train_loss), m._stream())

    def nxt(parts=_ptr(part), G=1, part_out=_ptr(part), part_cap=cap, n_out=C.byref(n)):
        return lib.coper_train_sync_next(h, parts, G, part_out, part_cap, n_out, m._stream())

    assert nxt() == ESTATE      # no step open
    assert begin(rows=2) == EINVAL and begin(rows=-1) == EINVAL
    assert begin(B_global=BG + 1) == EINVAL      # no multiple of B
    assert begin(off=BG - B + 1) == EINVAL and begin(off=-1) == EINVAL      # the shard leaves [0, B_global)
    assert begin(part_cap=2 * md["conv_num_channels"] - 1) == EINVAL
    assert begin(part_out=None) == EINVAL and begin(part_out=odd) == EINVAL and begin(n_out=None) == EINVAL
    assert begin(rows=1) == ESTATE      # outside the deferred-rows mode, as coper_train_rows_backward
    assert m.train_sync_phase == 0 and n.value in (-1, 0)
    assert begin() == 0 and n.value == 2 * md["conv_num_channels"] and m.train_sync_phase == 1
    # in the middle of a step
    assert _code(lambda: m.train_grads_export()) == ESTATE
    flat = torch.zeros(m.train_grads_layout()[1], device="cuda:0")
    assert _code(lambda: m.train_apply(flat)) == ESTATE and _code(lambda: m.train_apply()) == ESTATE
    assert nxt(G=0) == EINVAL and nxt(parts=None) == EINVAL and nxt(parts=odd) == EINVAL and nxt(n_out=None) == EINVAL
    assert nxt(part_out=None) == EINVAL and nxt(part_out=odd) == EINVAL and nxt(part_cap=2 * md["ent_emb_size"] - 1) == EINVAL
    assert m.train_sync_phase == 1      # (a refused argument leaves the step open)
    assert nxt() == 0 and n.value == 2 * md["ent_emb_size"] and m.train_sync_phase == 2
    m.train_backward(shard)      # a step-shaped call abandons the open step
    assert m.train_sync_phase == 0 and nxt() == ESTATE
    m.close()

    # the deferred-rows mode: rows = 0 is refused as coper_train_backward is, and the row calls refuse an open step
    m = _model(md, p0, True, ordered_rows=True, deferred_rows=True)
    assert _code(lambda: m.train_sync_begin(shard, BG, B)) == EUNSUPPORTED
    part_r, n_r = m.train_sync_begin(shard, BG, B, rows=True)
    assert n_r == 2 * md["conv_num_channels"]
    assert _code(lambda: m.train_rows_export()) == ESTATE
    small = torch.zeros(m.train_rows_layout()[1], device="cuda:0")
    assert _code(lambda: m.train_rows_apply(small)) == ESTATE
    m.close()

    # an entity-sharded state
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0", shard=(0, md["num_ent"]))
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=S.SEED, clip_norm=S.CLIP, deterministic=True, entity_sharded=True)
    assert _code(lambda: m.train_sync_begin(shard, BG, B)) == EUNSUPPORTED
    m.close()


# ------------------------------------------------------------------------------------------------ 6
def test_an_abandoned_step_leaves_no_trace_in_the_next():
    """a synchronised step abandoned in front of its third exchange, then train_step -- against a fresh handle loaded with the
    state the abandoned step left (it has moved Conv1BN's and FCBN's moving statistics) that runs the same train_step: every output and
    the whole state bit for bit."""
    md = S.md_for("cpg_linear")
    mode = TH.mode_of(deterministic=True)
    with TH.LiveBytes():
        H = TH.new_handle(md, (TH.p0_for(md), None), mode)
        try:
            batch = S.batch(md, "sampled", BG, L, BATCH_SEED)
            _, ns = _sync_backward([H], [shard_batch(batch, 1, 2)], stop_at=3)
            assert H.train_sync_phase == 3
            state = TH._save(H)
            nxt = S.batch(md, "sampled", 40, 37, 1001)
            got_h = TH._outs(H, H.train_step(nxt))
            assert H.train_sync_phase == 0
            F = TH.new_handle(md, state, mode)
            try:
                got_f = TH._outs(F, F.train_step(nxt))
            finally:
                F.close()
            TH.compare(got_h, got_f, "train_step behind an abandoned synchronised step")
        finally:
            H.close()
