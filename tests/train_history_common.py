"""Shared by tests/test_gpu_train_histories.py: a harness that runs a training call on a handle WITH a call history and on a fresh
handle loaded with that handle's state, and compares everything the call leaves.  Not a test module.

The training state keeps workspaces that grow on demand (the batch / lookup capacities and the buffers sized from them, the dense S,
the deterministic slabs, the split-K pool, the GEMM plane sets, the sort workspace, the deferred-row lists, the sharded score
buffers) and facts carried from call to call (the dense weights' recorded maximum, the exponent cache, which row list is the previous
one, pending gradients, claim bits owed a re-zero).  A result may depend on none of them: in the deterministic modes the same call
from the same variables, BN moving statistics, slots, powers and step counter leaves the same bits on any handle.

An OP is a tuple, one public call or one fixed group of calls of coper_amd.models.ConvE:
  ("S", B, L) ("D", B) ("C", B)      train_step on a sampled, dense 1-vs-all or CSR batch (tests/test_gpu_train_deterministic.py::_batch)
  ("F", form, B, L)                  train_forward(want_predictions=True, want_h=True); nothing may change
  ("BA", form, B, L)                 train_backward, train_apply()
  ("BEA", form, B, L)                train_backward, train_grads_export, train_apply(flat, scale=0.5)
  ("ROWS", B, L, imports, scale)     train_rows_backward, train_rows_export, [train_rows_import(first=True) of the second half of the
                                     block, train_rows_import(first=False) of its first two thirds, train_rows_export of the block,]
                                     train_rows_apply(small or None, scale) -- one op, because pending gradients are no part of a state
  ("IMPORT", n1, n2, scale)          train_rows_import(first=True) of n1 host-made rows, train_rows_import(first=False) of n2,
                                     train_rows_export of the block, train_rows_apply(host-made small, scale): no backward, so the
                                     imports alone size the row lists (rows_grow_keep in coper_train.hip)
  ("SYNC",)                          train_sync_rows
  ("ORDER", on) ("DEFER", on)        the mode switches
  ("REFUSED", form, B)               a 1-vs-all train_step that deferred rows refuses (include/coper_hip.h, "Deferred rows": "these are
                                     refused with COPER_EUNSUPPORTED ... the handle stays usable: 1-vs-all steps, dense or CSR")
  ("EVAL",)                          prepare() and the filtered ranks of 8 queries
The batch of op k of a history is drawn from seed 1000 + k."""
import gc

import numpy as np
import pytest
import torch

from coper_amd import data as cdata
from tests import shard_train_common as SC
from tests import test_gpu_train_deterministic as D
from tests.test_gpu_train_ordered import _outs, _save

SEED = D._SEED
CHUNK = 128      # one_vs_all_chunk: E = 211 is two chunks of a CSR step
EUNSUPPORTED = 7
_FORMS = {"S": "sampled", "D": "dense", "C": "csr"}


def p0_for(md):
    return {k: torch.as_tensor(np.array(v, np.float32)) for k, v in cdata.synthetic_params(md, seed=21, ent_std=0.1).items()}


def mode_of(deterministic=True, ordered=False, deferred=False):
    return dict(deterministic=deterministic, ordered=ordered, deferred=deferred)


def new_handle(md, state, mode):
    """A handle that has no call history: created, loaded with `state` = (variables and BN statistics, (slots, powers incl. the step
    counter) or None for a new optimizer) and put into `mode`."""
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: v.clone() for k, v in state[0].items()})
    m.train_init(seed=SEED, one_vs_all_chunk=CHUNK, deterministic=mode["deterministic"], ordered_rows=mode["ordered"],
                 deferred_rows=mode["deferred"])
    if state[1] is not None:
        m.load_optimizer_state(*state[1])
    return m


def state_bits(m):
    """The state of a handle as host arrays: variables, BN moving statistics, slots, powers and the step counter (behind a sync)."""
    tensors, (slots, powers) = _save(m)
    out = {"var/" + k: v.cpu().numpy() for k, v in tensors.items()}
    for leaf, parts in slots.items():
        for i, part in enumerate(parts):
            out["slot%d/%s" % (i, leaf)] = np.array(part)
    for k, v in powers.items():
        out["power/" + k] = np.float64(v)
    return out


def op_batch(md, op, k):
    kind = op[0]
    if kind in _FORMS:
        return D._batch(md, _FORMS[kind], op[1], op[2] if kind == "S" else 0, 1000 + k)
    if kind in ("F", "BA", "BEA"):
        return D._batch(md, op[1], op[2], op[3], 1000 + k)
    if kind == "ROWS":
        return D._batch(md, "sampled", op[1], op[2], 1000 + k)
    if kind == "REFUSED":
        return D._batch(md, op[1], op[2], 0, 1000 + k)
    return None


def _host(t):
    return t.cpu().numpy().copy()


def _rows_group(m, batch, imports, scale, out):
    loss = m.train_rows_backward(batch)
    small, ids, vals, count = m.train_rows_export()
    n = int(count.cpu()[0])
    out.update({"rows/small": _host(small), "rows/ids": _host(ids)[:n], "rows/vals": _host(vals)[:n], "rows/count": _host(count),
                "rows/pad_is_-1": np.int64((_host(ids)[n:] == -1).all())})
    for key, v in m.train_row_stats().items():
        out["rows/pending/" + key] = np.int64(v)
    if imports:
        half, two_thirds = slice(n // 2, n), slice(0, 2 * n // 3)
        m.train_rows_import(ids[half].clone(), vals[half].clone(), first=True)
        m.train_rows_import(ids[two_thirds].clone(), vals[two_thirds].clone(), first=False)
        _, ids2, vals2, count2 = m.train_rows_export(small=False)
        n2 = int(count2.cpu()[0])
        out.update({"rows2/ids": _host(ids2)[:n2], "rows2/vals": _host(vals2)[:n2], "rows2/count": _host(count2)})
        for key, v in m.train_row_stats().items():
            out["rows2/pending/" + key] = np.int64(v)
        m.train_rows_apply(small, scale)
    else:
        m.train_rows_apply(None, scale)
    return loss


def _import_group(m, md, k, n1, n2, scale, out):
    """Two host-made row blocks (ascending ids, n1 then n2 rows that overlap) and a host-made small vector: no backward is pending."""
    rng = np.random.default_rng(1000 + k)
    E, d = md["num_ent"], md["ent_emb_size"]
    layout, total, rs = m.train_rows_layout()
    for i, n in enumerate((n1, n2)):
        ids = np.sort(rng.choice(E, n, replace=False)).astype(np.int32)
        vals = np.zeros((n, rs), np.float32)
        vals[:, :d + 1] = rng.normal(0.0, 1e-3, (n, d + 1))
        m.train_rows_import(torch.as_tensor(ids).cuda(), torch.as_tensor(vals).cuda(), first=i == 0)
    _, ids2, vals2, count2 = m.train_rows_export(small=False)
    n = int(count2.cpu()[0])
    out.update({"rows2/ids": _host(ids2)[:n], "rows2/vals": _host(vals2)[:n], "rows2/count": _host(count2)})
    for key, v in m.train_row_stats().items():
        out["rows2/pending/" + key] = np.int64(v)
    small = np.zeros(total, np.float32)
    for off, cnt in layout.values():
        small[off:off + cnt] = rng.normal(0.0, 1e-3, cnt)
    m.train_rows_apply(torch.as_tensor(small).cuda(), scale)


def run_op(m, md, op, k, mode, quiet=False):
    """Runs op k of a history on `m` (and moves `mode` with a switch) -> everything it leaves as {name: host array}.  quiet: nothing is
    read back but the loss the op returns (a read of the state brings deferred rows current)."""
    from coper_amd._lib import CoperError
    kind, batch, out = op[0], op_batch(md, op, k), {}
    if kind in _FORMS:
        loss = m.train_step(batch)
    elif kind == "F":
        before = None if quiet else state_bits(m)
        loss, pred, hv = m.train_forward(batch, want_predictions=True, want_h=True)
        out.update({"forward/pred": _host(pred), "forward/h": _host(hv), "loss": _host(loss)})
        if not quiet:
            D._assert_same_bits(state_bits(m), before, "a forward changed the state: op %d %r" % (k, op))
        return out
    elif kind == "BA":
        loss = m.train_backward(batch)
        m.train_apply()
    elif kind == "BEA":
        loss = m.train_backward(batch)
        flat = m.train_grads_export()
        out["flat"] = _host(flat)
        m.train_apply(flat, scale=0.5)
    elif kind == "ROWS":
        loss = _rows_group(m, batch, op[3], op[4], out)
    elif kind == "IMPORT":
        # (the gradient buffers of the small leaves hold what an EARLIER backward left: no output of this op, so the state is compared)
        _import_group(m, md, k, op[1], op[2], op[3], out)
        if quiet:
            return {}
        out.update(state_bits(m))
        for key, v in m.train_row_stats().items():
            out["rows/" + key] = np.int64(v)
        return out
    elif kind == "REFUSED":
        with pytest.raises(CoperError) as bad:
            m.train_step(batch)
        assert bad.value.code == EUNSUPPORTED, bad.value
        return {} if quiet else state_bits(m)
    elif kind == "SYNC":
        m.train_sync_rows()
        return {} if quiet else state_bits(m)
    elif kind == "ORDER":
        m.train_order_rows(op[1])
        mode["ordered"] = bool(op[1])
        return {} if quiet else state_bits(m)
    elif kind == "DEFER":
        m.train_defer_rows(op[1])
        mode["deferred"] = bool(op[1])
        return {} if quiet else state_bits(m)
    elif kind == "EVAL":
        q = cdata.synthetic_queries(md, 8, seed=1000 + k)
        m.prepare()
        ranks, n_equal = m.rank_pass(q["e1"], q["rel"], q["e2"], q["filt_indptr"], q["filt_idx"])
        return {"eval/ranks": _host(ranks), "eval/n_equal": _host(n_equal)}
    else:
        raise ValueError(op)
    if quiet:
        out = {"loss": _host(loss)}
    else:
        out.update(_outs(m, loss))      # loss, every gradient, the norm, every variable, every slot, the powers, the row statistics
    return out


def compare(got_h, got_f, what):
    """The history handle's outputs against the fresh handle's: the same names, types, shapes and bits."""
    D._assert_same_bits(got_h, got_f, what)


class LiveBytes(object):
    """`with LiveBytes():` -- the library's allocation ledger is back at its value once every handle of the block is closed."""

    def __enter__(self):
        from coper_amd import _lib
        self.lib = _lib.load()
        gc.collect()      # handles earlier tests dropped without close()
        self.base = self.lib.coper_live_device_bytes()
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            gc.collect()
            live = self.lib.coper_live_device_bytes()
            assert live == self.base, (self.base, live)
        return False


def run_checkpointed(md, mode0, ops):
    """Protocol 1.  Before op k on the history handle H its state is taken; the op runs on H; a fresh handle F with H's switches is
    loaded with that state, runs the same op and is closed; everything the op leaves is bit-identical."""
    with LiveBytes():
        mode = dict(mode0)
        H = new_handle(md, (p0_for(md), None), mode)
        try:
            for k, op in enumerate(ops):
                state, mode_f = _save(H), dict(mode)
                got_h = run_op(H, md, op, k, mode)
                F = new_handle(md, state, mode_f)
                try:
                    got_f = run_op(F, md, op, k, mode_f)
                finally:
                    F.close()
                assert mode_f == mode
                compare(got_h, got_f, "op %d %r: the handle with a history against a fresh one" % (k, op))
        finally:
            H.close()


def run_end_to_end(md, mode0, ops):
    """Protocol 2.  H runs the whole history and nothing is read in between but each op's loss; a chain of fresh handles runs the same
    ops, F_k created from F_{k-1}'s state after its op -> ([loss of H per op], [loss of the chain per op], H's state, the chain's)."""
    with LiveBytes():
        mode = dict(mode0)
        H = new_handle(md, (p0_for(md), None), mode)
        try:
            losses_h = [run_op(H, md, op, k, mode, quiet=True).get("loss") for k, op in enumerate(ops)]
            end_h = state_bits(H)
        finally:
            H.close()
        mode, state, losses_f = dict(mode0), (p0_for(md), None), []
        for k, op in enumerate(ops):
            F = new_handle(md, state, mode)
            try:
                losses_f.append(run_op(F, md, op, k, mode, quiet=True).get("loss"))
                state = _save(F)
                if k == len(ops) - 1:
                    end_f = state_bits(F)
            finally:
                F.close()
    return losses_h, losses_f, end_h, end_f


def run_twins(md, mode0, prefix, ops):
    """Protocol 2 where rows fall several updates behind.  A chain of fresh handles starts every op with every row current, so there
    the header promises rounding, not bits ("p is rounded once per gap instead of once per update").  What it promises to the bit is
    "between handles with different histories (a row list or workspace that grew earlier from a larger batch)": twin A is fresh, twin B
    first runs `prefix` and is put back to the initial state (every row current, as on A); both then run `ops` with nothing read in
    between but the losses -> ([loss of A per op], [loss of B per op], A's state, B's)."""
    from tests.test_gpu_train_ordered import _restore
    with LiveBytes():
        twins = [new_handle(md, (p0_for(md), None), mode0) for _ in range(2)]
        try:
            start = _save(twins[1])
            mode = dict(mode0)
            for k, op in enumerate(prefix):
                run_op(twins[1], md, op, 500 + k, mode, quiet=True)
            assert mode == mode0
            _restore(twins[1], start)
            losses, ends = [], []
            for m in twins:
                mode = dict(mode0)
                losses.append([run_op(m, md, op, k, mode, quiet=True).get("loss") for k, op in enumerate(ops)])
                ends.append(state_bits(m))
        finally:
            for m in twins:
                m.close()
    return losses[0], losses[1], ends[0], ends[1]


def max_row_gap(md, mode0, ops):
    """The largest number of updates a row of ent_emb / pred_bias is behind when something brings it current, over a history that is
    run WITHOUT reads (protocol 2), worked out on the host from the batches: a step or a rows group brings the rows it names current
    and leaves every other row one more update behind; a sync, leaving the mode, and the read at the end bring all rows current."""
    E = md["num_ent"]
    behind, deferred, worst = np.zeros(E, np.int64), mode0["deferred"], 0
    for k, op in enumerate(ops):
        kind = op[0]
        if kind in ("S", "ROWS"):
            if deferred:
                batch = op_batch(md, op, k)
                ids = np.concatenate([np.asarray(batch["e1"]).reshape(-1), np.asarray(batch["lookup_values"]).reshape(-1)]).astype(np.int64)
                ids[(ids < 0) | (ids >= E)] = 0
                named = np.zeros(E, bool)
                named[ids] = True
                worst = max(worst, int(behind[named].max()))
                behind[named] = 0
                behind[~named] += 1
        elif kind in ("SYNC", "DEFER"):
            worst = max(worst, int(behind.max()))
            behind[:] = 0
            if kind == "DEFER":
                deferred = bool(op[1])
        elif kind != "REFUSED":
            raise ValueError(op)
    return max(worst, int(behind.max()))


# ---- entity-sharded histories (coper_amd.parallel.EntityShardedTrainer; tests/shard_train_common.py)
def _shards_from_state(md, states, bounds):
    from coper_amd.models import ConvE
    models = []
    for (tensors, (slots, powers)), (lo, hi) in zip(states, bounds):
        m = ConvE(md, device="cuda:0", shard=(lo, hi))
        m.load_parameters({k: v.clone() for k, v in tensors.items()}, global_rows=False)      # (the shard's own rows)
        m.train_init(seed=SC.SEED, clip_norm=SC.CLIP_OFF, deterministic=True, entity_sharded=True, one_vs_all_chunk=CHUNK)
        m.load_optimizer_state(slots, powers)
        models.append(m)
    return models


def run_sharded(md, bounds, ops):
    """The checkpointed protocol over EntityShardedTrainer(models=[...]).step: before each step a fresh trainer is built from the
    shards' states; SC.snapshot and the loss are bit-identical after it."""
    from coper_amd.parallel import EntityShardedTrainer
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    with LiveBytes():
        hist = [SC.shard_model(md, p0, lo, hi, SC.CLIP_OFF, chunk=CHUNK) for lo, hi in bounds]
        try:
            trainer = EntityShardedTrainer(models=hist)
            for k, op in enumerate(ops):
                batch = op_batch(md, op, k)
                states = [({n: v.clone() for n, v in m._tensors.items()}, m.optimizer_state()) for m in hist]
                loss_h = _host(trainer.step(batch))
                fresh = _shards_from_state(md, states, bounds)
                try:
                    loss_f = _host(EntityShardedTrainer(models=fresh).step(batch))
                    snap_f = SC.snapshot(fresh)
                finally:
                    for m in fresh:
                        m.close()
                what = "sharded op %d %r" % (k, op)
                assert loss_h.tobytes() == loss_f.tobytes(), (what, loss_h, loss_f)
                SC.same_bits(SC.snapshot(hist), snap_f, what)
        finally:
            for m in hist:
                m.close()
