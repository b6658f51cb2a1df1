"""Data-parallel training and gradient accumulation over the split step (include/coper_hip.h: coper_train_backward |
coper_train_grads_export | coper_train_apply).

Every rank holds a full replica of the model (`ConvE` after `train_init`).  An update is: per micro-batch a backward pass and an
export that ADDS its gradient into one flat vector, ONE all-reduce (sum) of that vector over the ranks, then the optimizer on the sum
scaled by 1 / (ranks * micro-batches).  The replicas start equal (rank 0's state is broadcast) and stay equal, because every rank
applies the same bytes.  The all-reduce does not overlap the backward pass.  Batch statistics are per rank unless the trainer is built
with `sync_bn=True`: then every micro-batch's backward is the phased step of include/coper_hip.h, "Synchronised batch statistics"
(DESIGN.md 6.13), and an update is the reference's update on the whole batch.

Entity-sharded (model-parallel) 1-vs-all training is `EntityShardedTrainer` below: the entity table, its gradients and
slots split over the ranks, the encoder replicated; sampled labels on a sharded table are not built.

In the deferred-rows mode (coper_train_defer_rows) the same update is made from coper_train_rows_backward | _export | _import | _apply:
a small flat vector for everything but ent_emb / pred_bias, and row blocks (ids, gradient rows) for those two.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .models import _ptr

_PER_SAMPLE = ("e1", "rel", "lookup_values", "e2_multi", "lab_row")


def shard_batch(batch, rank, world):
    """Rank `rank`'s even slice of a training batch dict, in any of the three label forms `ConvE.train_step` takes: sampled
    (`lookup_values`, `e2_multi` [B, L]), dense 1-vs-all (`e2_multi` [B, num_ent]) and sparse 1-vs-all (`lab_indptr`, `lab_idx`,
    optional `lab_row`).  A sparse batch keeps its label table -- the same objects, not copies -- and slices `lab_row` (a batch
    without one gets the row numbers of the slice).  B % world != 0 raises ValueError: every rank reports the MEAN loss of its
    shard, and the mean of shard means is the batch mean only for equal shards."""
    rank, world = int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("shard_batch: rank %d of world %d" % (rank, world))
    B = len(batch["e1"])
    if B % world:
        raise ValueError("shard_batch: a batch of %d does not split evenly over %d ranks" % (B, world))
    n = B // world
    lo, hi = rank * n, (rank + 1) * n
    out = {k: (v[lo:hi] if k in _PER_SAMPLE and v is not None else v) for k, v in batch.items()}
    if "e2_multi" not in batch and "lab_indptr" in batch and batch.get("lab_row", None) is None:
        ip = batch["lab_indptr"]
        out["lab_row"] = (torch.arange(lo, hi, dtype=torch.int64, device=ip.device) if isinstance(ip, torch.Tensor)
                          else np.arange(lo, hi, dtype=np.int64))
    return out


class DataParallelTrainer(object):
    """`DataParallelTrainer(model, group=None, micro_batches=1, sync_bn=False)`: one replica per rank of a `torch.distributed` process group
    (`group=None`: the default group; no initialised process group at all: one process, plain gradient accumulation).

    Construction broadcasts rank 0's variables (BN moving statistics included), AMSGrad slots, beta powers and dropout counter.
    `step(batches)` takes this rank's list of `micro_batches` local batches and makes one update:

      * per micro-batch `train_backward` + `train_grads_export(accumulate)` into one flat vector;
      * ONE `all_reduce(SUM)` of the flat vector;
      * `train_apply(flat, 1 / (world * micro_batches))`: the clip acts on the norm of the MEAN gradient;
      * the BN moving statistics, which every rank updated from its own batches, are averaged over the ranks in one small
        all-reduce (the loss rides in it), so the replicas stay equal.

    Batch statistics are per rank and per micro-batch by default, as in torch's DistributedDataParallel without SyncBN: a rank
    normalises by the statistics of the micro-batch in front of it, never by the global batch's.  The gradient is therefore the mean of
    the micro-batch gradients, not the gradient of the concatenated batch, wherever batch statistics are on.

    SYNCHRONISED BATCH STATISTICS.  `sync_bn=True`: every micro-batch's backward is `train_sync_begin` + four `train_sync_next`, the
    ranks' shares of each batch-wide sum gathered in rank order in between (four small all-gathers of at most
    2 max(conv_num_channels, ent_emb_size) doubles; over gloo staged through the host).  Rank r's micro-batch i is samples
    [r B, (r + 1) B) of a batch of world * B samples -- the ranks' i-th micro-batches, `shard_batch`'s slices of one batch -- so Conv1BN
    and FCBN normalise by that whole batch and the dropout masks are the whole batch's: with micro_batches == 1 the update is ONE step on
    the concatenated batch.  Micro-batch i is synchronised over the ranks' i-th micro-batches, NOT across micro-batches: with
    micro_batches > 1 the gradient is the mean of the gradients of M batches of world * B samples.  Every rank must pass the same B.  The
    moving statistics are equal on every rank by construction and are not averaged; the loss still rides in the small all-reduce.  Both
    routes take it (the sparse one through `train_sync_begin(rows=True)`).  Refused by the library: a generator with hidden layers and
    context BN.  One seed on every rank (`train_init(seed=s)`): the masks are already a function of the sample's global position.

    Dropout masks are a function of (seed, dropout counter, element): ranks draw DIFFERENT masks only if the caller gave them
    different seeds -- `model.train_init(seed=s + rank)`.  With one seed every rank drops the same positions of its own shard.

    The averaged moving statistics are written into the caller's tensors in place.  That moves their version counters, and the
    model registers them again (coper_set_param); registering a moving statistic again does not discard what the optimizer's
    last pass recorded about the dense weights (their largest magnitude, which the next step's operand packing scales by).

    THE SPARSE ROUTE.  A model in the deferred-rows mode (`train_init(deferred_rows=True)`, `model.train_rows_deferred == 1` at
    construction) never forms the dense gradient of ent_emb / pred_bias, so there is no flat vector to all-reduce.  `step` then makes
    the update from the mode's own split step (include/coper_hip.h, "Deferred rows: the step in calls"):

      * per micro-batch i `train_rows_backward` + `train_rows_export`: the SMALL flat vector (every leaf but the two tables)
        accumulates in `flat`, the batch's rows and their gradient rows go into slot i of an [M, cap] / [M, cap, rs] pair of buffers;
      * ONE `all_reduce(SUM)` of the small vector;
      * one `all_gather` of the M block lengths and ONE HOST READ of their maximum `mx` -- the only host synchronisation of an update.
        It buys gathering `ids[:, :mx]` / `vals[:, :mx]` instead of cap = B (L + 1) rows per rank and micro-batch every time;
      * every rank imports ALL world * M blocks, its own included, from the gathered buffers in ascending (rank, micro-batch) order,
        the first with `first=True`: every replica adds the same bytes in the same order, one writer per element, no float atomics --
        the replicas' table gradients are equal byte for byte (`gathered` keeps the last update's buffers);
      * `train_rows_apply(flat, 1 / (world * micro_batches))`; moving statistics and loss as above.

    The replicas' VARIABLES are not claimed equal to the bit on this route: the mode's squared norm is summed by unordered atomics.
    When `model.train_rows_ordered` is 1 (`train_init(deterministic=True, ordered_rows=True, deferred_rows=True)`; include/coper_hip.h,
    "Ordered rows") they ARE: the blocks come in ascending row id, the pending list is sorted before the norm reads it and the norm is
    summed in one fixed order, so replicas that import the same blocks in the same order and apply the same small vector end
    byte-identical in every variable, slot, power and row word.  No new route: the one above, chosen by `train_rows_deferred`.
    Construction brings every row current (`train_sync_rows`) before the raw tables are broadcast.  Over gloo, which gathers host
    tensors only, the blocks are staged through the host: ranks sharing a GPU are a correctness run, and multi-GPU scaling of this route
    has not been measured.  Sampled batches only (the mode refuses 1-vs-all)."""

    def __init__(self, model, group=None, micro_batches=1, sync_bn=False):
        import torch.distributed as dist
        if getattr(model, "_train_loss", None) is None:
            raise _lib.CoperError(5, "call train_init() first")
        self.model = model
        self.micro_batches = int(micro_batches)
        if self.micro_batches < 1:
            raise ValueError("micro_batches >= 1")
        self._dist = dist if dist.is_available() and dist.is_initialized() else None
        if self._dist is None and group is not None:
            raise ValueError("a process group needs torch.distributed to be initialised")
        self.group = group
        self.world = self._dist.get_world_size(group) if self._dist else 1
        self.rank = self._dist.get_rank(group) if self._dist else 0
        self.sparse = model.train_rows_deferred == 1      # the deferred-rows mode: the sparse route (class docstring)
        self.sync_bn = bool(sync_bn)
        if self.sparse:
            self.layout, total, self.row_stride = model.train_rows_layout()
            self._ids = self._vals = None                 # [M, cap] / [M, cap, rs]: micro-batch i's row block in slot i
            self._counts = torch.zeros(self.micro_batches, device=model.device, dtype=torch.int32)
            self.gathered = None                          # the last update's (ids [W, M, mx], vals [W, M, mx, rs]) as every rank imported them
        else:
            self.layout, total = model.train_grads_layout()
        self.flat = torch.zeros(total, device=model.device, dtype=torch.float32)
        self._stat_names = [k for k in model._tensors if k.endswith(("moving_mean", "moving_variance"))]
        n_stats = sum(model._tensors[k].numel() for k in self._stat_names)
        self._small = torch.zeros(n_stats + 1, device=model.device, dtype=torch.float32)      # moving statistics | loss
        if self.world > 1:
            self._broadcast_state()

    # ---- construction
    def _src(self):
        return self._dist.get_global_rank(self.group, 0) if self.group is not None else 0

    def _broadcast_state(self):
        m, dist, src = self.model, self._dist, self._src()
        m.train_sync_rows()      # (deferred rows: the raw ent_emb / pred_bias tensors are current only after a sync)
        for t in m._tensors.values():
            dist.broadcast(t, src=src, group=self.group)
        # (whether a collective into a tensor moves its version counter is the backend's business: register every tensor again --
        #  stale inference caches, entity maximum and carried weight maximum go with it)
        m.parameters_changed()
        n = C.c_int64()
        for leaf in m.trainable_leaves():
            for which in range(3):
                _lib.check(m._h, m._lib.coper_train_slot(m._h, leaf.encode(), which, None, 0, 0, C.byref(n), m._stream()))
                buf = torch.empty(n.value, device=m.device, dtype=torch.float32)
                _lib.check(m._h, m._lib.coper_train_slot(m._h, leaf.encode(), which, _ptr(buf), n.value, 0, C.byref(n), m._stream()))
                dist.broadcast(buf, src=src, group=self.group)
                _lib.check(m._h, m._lib.coper_train_slot(m._h, leaf.encode(), which, _ptr(buf), n.value, 1, C.byref(n), m._stream()))
                torch.cuda.current_stream(m.device).synchronize()      # buf may be freed after this
        b1, b2, st = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(m._h, m._lib.coper_train_powers(m._h, None, None, None, C.byref(b1), C.byref(b2), C.byref(st)))
        pw = torch.tensor([b1.value, b2.value, float(st.value)], dtype=torch.float64, device=m.device)
        dist.broadcast(pw, src=src, group=self.group)
        b1v, b2v, stv = pw.cpu().tolist()
        b1, b2, st = C.c_double(b1v), C.c_double(b2v), C.c_int64(int(stv))
        _lib.check(m._h, m._lib.coper_train_powers(m._h, C.byref(b1), C.byref(b2), C.byref(st), None, None, None))

    # ---- one update
    def step(self, batches):
        """One update from this rank's `micro_batches` local batches (a list; a single dict when micro_batches == 1).  Returns
        the loss averaged over ranks and micro-batches as a 1-element device tensor (no synchronisation of the host)."""
        m = self.model
        if isinstance(batches, dict):
            batches = [batches]
        if len(batches) != self.micro_batches:
            raise ValueError("step: %d local batches, micro_batches = %d" % (len(batches), self.micro_batches))
        if self.sparse:
            return self._step_rows(batches)
        small = self._small
        loss = small[-1:]
        for i, b in enumerate(batches):
            li = self._backward_sync(b, rows=False) if self.sync_bn else m.train_backward(b)
            m.train_grads_export(self.flat, accumulate=i > 0)
            if i:
                loss += li
            else:
                loss.copy_(li)
        if self.world > 1:
            dist = self._dist
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
        self._average_stats()
        m.train_apply(self.flat, 1.0 / (self.world * self.micro_batches))
        return loss / float(self.world * self.micro_batches)

    def _backward_sync(self, batch, rows):
        """One micro-batch's backward with batch statistics over the ranks' shards (class docstring): the phase loop, the ranks' parts
        gathered in rank order between the calls.  Returns the loss of this rank's shard as a 1-element device tensor."""
        m, B = self.model, len(batch["e1"])
        part, n = m.train_sync_begin(batch, B_global=self.world * B, sample_offset=self.rank * B, rows=rows)
        while n:
            parts = self._gather(part[:n]) if self.world > 1 else part[:n].unsqueeze(0)
            part, n = m.train_sync_next(parts)
        return m.train_sync_loss

    def _average_stats(self):
        """The BN moving statistics averaged over the ranks in one small all-reduce, written back in place; the loss rides in it.
        sync_bn: the statistics are equal on every rank already -- the loss alone is summed."""
        m, small = self.model, self._small
        if self.world > 1 and self.sync_bn:
            self._dist.all_reduce(small[-1:], op=self._dist.ReduceOp.SUM, group=self.group)
        elif self.world > 1:
            dist = self._dist
            at = 0
            for k in self._stat_names:
                t = m._tensors[k]
                small[at:at + t.numel()].copy_(t.reshape(-1))
                at += t.numel()
            dist.all_reduce(small, op=dist.ReduceOp.SUM, group=self.group)
            small[:-1] /= float(self.world)
            at = 0
            for k in self._stat_names:
                t = m._tensors[k]
                t.copy_(small[at:at + t.numel()].reshape(t.shape))
                at += t.numel()

    # ---- one update in the deferred-rows mode
    def _gather(self, t):
        """`t` of every rank, stacked [world, ...] in rank order, on the model's device.  gloo gathers host tensors only: there the
        tensor is staged through the host (ranks sharing a GPU over gloo are a correctness run)."""
        dist = self._dist
        if dist.get_backend(self.group) == "nccl":
            out = torch.empty((self.world,) + tuple(t.shape), device=t.device, dtype=t.dtype)
            dist.all_gather_into_tensor(out, t.contiguous(), group=self.group)
            return out
        host = t.cpu().contiguous()
        parts = [torch.empty_like(host) for _ in range(self.world)]
        dist.all_gather(parts, host, group=self.group)
        return torch.stack(parts).to(t.device)

    def _step_rows(self, batches):
        """The sparse route (class docstring): the small flat vector is all-reduced, the tables' gradients travel as row blocks."""
        m, M, rs = self.model, self.micro_batches, self.row_stride
        small = self._small
        loss = small[-1:]
        # the bound of a backward's row list, min(B (L + 1), num_ent) (a batch without sampled labels: train_rows_backward refuses it)
        cap = max(min(len(b["e1"]) * (int(b["e2_multi"].shape[1]) + 1), m.num_ent) if "e2_multi" in b else 1 for b in batches)
        if self._ids is None or self._ids.shape[1] < cap:
            self._ids = torch.full((M, cap), -1, device=m.device, dtype=torch.int32)
            self._vals = torch.zeros((M, cap, rs), device=m.device, dtype=torch.float32)
        for i, b in enumerate(batches):
            li = self._backward_sync(b, rows=True) if self.sync_bn else m.train_rows_backward(b)
            cnt = m.train_rows_export(self.flat, accumulate=i > 0, ids=self._ids[i], vals=self._vals[i])[3]
            self._counts[i:i + 1].copy_(cnt)
            if i:
                loss += li
            else:
                loss.copy_(li)
        if self.world > 1:
            dist = self._dist
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
            mx = int(self._gather(self._counts).max().item())      # the ONE host synchronisation of an update
            ids, vals = self._gather(self._ids[:, :mx]), self._gather(self._vals[:, :mx])
            self.gathered = (ids, vals)
            blocks = [(ids[r, i], vals[r, i]) for r in range(self.world) for i in range(M)]
        else:
            blocks = [(self._ids[i], self._vals[i]) for i in range(M)]      # (whole slots: entries behind a block's count are padding)
        for j, (bi, bv) in enumerate(blocks):      # ascending (rank, micro-batch) on every rank: the same bytes in the same order
            m.train_rows_import(bi, bv, first=j == 0)
        self._average_stats()
        m.train_rows_apply(self.flat, 1.0 / (self.world * M))
        return loss / float(self.world * M)


class EntityShardedTrainer(object):
    """Entity-sharded (model-parallel) training, 1-vs-all from sparse labels or from sampled batches (include/coper_hip.h,
    "Entity-sharded training").  Rank g of G holds rows [lo_g, hi_g) of ent_emb / pred_bias with their gradients and AMSGrad slots
    (`ConvE(md, shard=(lo, hi))` + `train_init(deterministic=True, entity_sharded=True)`); every other leaf is replicated and stays
    byte-identical on every rank WITHOUT an exchange, because the deterministic mode makes the encoder a function of its inputs.

      * `EntityShardedTrainer(model, group=None)`: one shard per process of a `torch.distributed` group;
      * `EntityShardedTrainer(models=[m_0, ..., m_{G-1}])`: the G shards in one process; the exchanges are torch ops in rank order.

    Both forms leave the same bytes.  Construction checks that the shards' bounds tile [0, num_ent) in rank order and that seed,
    hyper-parameters, dropout counter and beta powers are equal on every rank, and raises ValueError otherwise.

    `step(batch)` takes the SAME batch on every rank -- `e1`, `rel` [B] and either `lab_indptr`, `lab_idx` (+ `lab_row`), as
    `ConvE.train_step` takes sparse 1-vs-all labels, or a sampled batch, `lookup_values` int32 [B, L] of global ids with `e2_multi`
    float [B, L] -- and makes one update (a step may use another label form than the step before):

      1. each rank gathers the e1 rows it holds (zero rows for the others); all-reduce: the [B, d] input rows (one non-zero addend
         per element: exact);
      2. `train_shard_forward`: the replicated encoder up to h;
      3. `train_shard_score` (sparse 1-vs-all: the scorer over the own rows) or `train_shard_score_lookup` (sampled: the scorer over
         the batch's entries whose row this shard holds, the table gradient by the ordered-rows route) -- this shard's table
         gradients, its share of dh and of the loss;
      4. all-gather of the [B, d] shares and of the loss doubles;
      5. `train_shard_backward`: the shares folded in rank order, the encoder's backward, the owned e1 rows, this shard's squared norm;
      6. all-gather of the G doubles;
      7. `train_shard_apply`: clip by the global norm, AMSGrad over the small leaves and the own rows.

    Nothing table-sized or logit-sized moves.  Returns the batch loss as a 1-element device tensor (per rank; a list in the
    in-process form would hold G equal values, so rank 0's is returned).  gloo, which moves host tensors only, is staged through the
    host as `DataParallelTrainer._gather` does.

    DEFERRED ROWS (`train_init(deterministic=True, entity_sharded=True, deferred_rows=True)` on every rank): sampled steps
    whose table work follows the batch instead of the shard's rows.  The seven steps and the three exchanges are the same; step 1 hands
    out rows as of the current update although the table may hold them several updates behind, step 3 lists the owned rows the batch
    names and brings them current, steps 5 and 7 take the norm and the update over that list.  Construction also compares the mode and
    its update counter across ranks (ValueError on a mismatch); `step` raises ValueError for a sparse 1-vs-all batch in the mode;
    `sync_rows()` brings every owned row current (the registered tables are current only then, as on a whole-table handle).  Both
    trainer forms leave the same bytes in the mode too.

    `forward(batch, want_predictions=False, want_h=False)` looks at a batch without an update: the loss, the train-mode logits and h
    from one call per rank (`ConvE.train_shard_forward_only`) between the gather of 1. and an all-gather of G doubles, with nothing
    written -- also in the deferred-rows mode, where the owned rows are read as of the current update and stay as they are in the table.

    Not built: dense [B, num_ent] labels, the row-block split step on a shard, the default (non-deterministic) mode, a batch split over
    ranks, overlap of the exchanges with compute; scaling with real RCCL exchanges has not been measured."""

    def __init__(self, model=None, group=None, models=None):
        import torch.distributed as dist
        if (model is None) == (models is None):
            raise ValueError("EntityShardedTrainer(model, group) or EntityShardedTrainer(models=[...])")
        self.local = list(models) if models is not None else [model]
        self._in_process = models is not None
        if not self.local:
            raise ValueError("EntityShardedTrainer: no models")
        for m in self.local:
            if getattr(m, "_train_loss", None) is None:
                raise _lib.CoperError(5, "call train_init(deterministic=True, entity_sharded=True) first")
            if m.train_sharded != 1:
                raise ValueError("EntityShardedTrainer: a model whose training state is not entity-sharded (train_init(entity_sharded=True))")
        self._dist = None
        self.group = group
        if models is None:
            self._dist = dist if dist.is_available() and dist.is_initialized() else None
            if self._dist is None and group is not None:
                raise ValueError("a process group needs torch.distributed to be initialised")
        elif group is not None:
            raise ValueError("EntityShardedTrainer(models=[...]) takes no process group")
        self.world = self._dist.get_world_size(group) if self._dist else len(self.local)
        self.rank = self._dist.get_rank(group) if self._dist else 0
        self._check_ranks()

    # ---- construction
    @staticmethod
    def _describe(m):
        """What must agree across ranks, and the bounds, as float64: [lo, hi, num_ent, hyper-parameters ..., beta powers, counter]."""
        b1, b2, st = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(m._h, m._lib.coper_train_powers(m._h, None, None, None, C.byref(b1), C.byref(b2), C.byref(st)))
        return ([float(m.shard[0]), float(m.shard[1]), float(m.num_ent)] + [float(v) for v in m._train_cfg] + [b1.value, b2.value, float(st.value)]
                + [float(m.train_rows_deferred), float(m.train_rows_updates)])      # (the last two: the deferred-rows mode, its update counter)

    def _check_ranks(self):
        mine = torch.tensor([self._describe(m) for m in self.local], dtype=torch.float64)
        if self._dist is not None:
            parts = [torch.empty_like(mine) for _ in range(self.world)]
            if self._dist.get_backend(self.group) == "nccl":
                dev = self.local[0].device
                parts = [p.to(dev) for p in parts]
                self._dist.all_gather(parts, mine.to(dev), group=self.group)
                parts = [p.cpu() for p in parts]
            else:
                self._dist.all_gather(parts, mine, group=self.group)
            mine = torch.cat(parts)
        rows = mine.tolist()
        at = 0.0
        for g, r in enumerate(rows):
            if r[0] != at or r[1] <= r[0]:
                raise ValueError("EntityShardedTrainer: the shards do not tile [0, num_ent) in rank order (rank %d holds [%d, %d))" % (g, r[0], r[1]))
            at = r[1]
            if r[-2:] != rows[0][-2:]:
                raise ValueError("EntityShardedTrainer: rank %d differs from rank 0 in the deferred-rows mode (train_defer_rows) or in its "
                                 "update counter" % g)
            if r[2:] != rows[0][2:]:
                raise ValueError("EntityShardedTrainer: rank %d differs from rank 0 in seed, hyper-parameters, dropout counter or beta powers" % g)
        if at != rows[0][2]:
            raise ValueError("EntityShardedTrainer: the shards end at %d of %d entities" % (at, rows[0][2]))

    # ---- the exchanges
    def _gather(self, t):
        """`t` of every rank stacked [world, ...] in rank order on t's device (process form)."""
        dist = self._dist
        if dist.get_backend(self.group) == "nccl":
            out = torch.empty((self.world,) + tuple(t.shape), device=t.device, dtype=t.dtype)
            dist.all_gather_into_tensor(out, t.contiguous(), group=self.group)
            return out
        host = t.cpu().contiguous()
        parts = [torch.empty_like(host) for _ in range(self.world)]
        dist.all_gather(parts, host, group=self.group)
        return torch.stack(parts).to(t.device)

    def _sum(self, t):
        """The sum of `t` over the ranks (process form; every element has one non-zero addend: exact in any order)."""
        dist = self._dist
        if dist.get_backend(self.group) == "nccl":
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
            return t
        host = t.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.group)
        return host.to(t.device)

    def _exchange(self, parts, reduce=False):
        """parts[i]: local model i's tensor.  Returns per local model the stacked [world, ...] tensor (or the sum) on its device."""
        if self._dist is not None and self.world > 1:
            return [self._sum(parts[0]) if reduce else self._gather(parts[0])]
        out = []
        for m in self.local:
            mine = [p.to(m.device) for p in parts]      # rank order
            if reduce:
                acc = mine[0].clone()
                for p in mine[1:]:
                    acc += p
                out.append(acc)
            else:
                out.append(torch.stack(mine))
        return out

    # ---- one update
    def step(self, batch):
        ms = self.local
        lv = batch.get("lookup_values", None)
        sampled = "e2_multi" in batch and lv is not None and np.ndim(lv) == 2 and np.shape(lv)[1] > 0      # (data.py: [B, 0] means 1-vs-all)
        if not sampled and ("lab_indptr" not in batch or "e2_multi" in batch):
            raise ValueError("EntityShardedTrainer.step: a 1-vs-all batch with sparse labels (lab_indptr, lab_idx [, lab_row]) or a sampled "
                             "batch (lookup_values, e2_multi [B, L]); dense e2_multi [B, num_ent] is not served")
        if not sampled and any(m.train_rows_deferred == 1 for m in ms):
            raise ValueError("EntityShardedTrainer.step: the models are in the deferred-rows mode, which serves sampled batches only (a 1-vs-all "
                             "step has a gradient in every row)")
        B = len(batch["e1"])
        d = ms[0].ent_emb_size
        rows = self._exchange([m.train_shard_gather(batch["e1"]) for m in ms], reduce=True)                      # 1
        dh, ls, sq = [], [], []
        for m, r in zip(ms, rows):
            m.train_shard_forward(batch["e1"], batch["rel"], r)                                                   # 2
            dh.append(torch.empty((B, d), device=m.device, dtype=torch.float32))
            ls.append(torch.empty(1, device=m.device, dtype=torch.float64))
            sq.append(torch.empty(1, device=m.device, dtype=torch.float64))
            (m.train_shard_score_lookup if sampled else m.train_shard_score)(batch, B, dh[-1], ls[-1])            # 3
        dh_all, ls_all = self._exchange(dh), self._exchange(ls)                                                   # 4
        losses = [m.train_shard_backward(a, l.reshape(-1), s) for m, a, l, s in zip(ms, dh_all, ls_all, sq)]      # 5
        sq_all = self._exchange(sq)                                                                               # 6
        for m, s in zip(ms, sq_all):
            m.train_shard_apply(s.reshape(-1))                                                                    # 7
        return losses[0]

    # ---- a batch looked at, nothing updated
    def forward(self, batch, want_predictions=False, want_h=False):
        """The loss (and on request the train-mode logits and h) of `batch` as a step on it would see them, with NOTHING written on any
        rank: no variable, moving statistic, gradient, slot, dropout counter or deferred-rows word -- the held-out loss
        of a sharded run.  Between steps only.  The same batch on every rank, as `step` takes it:

          1. the gather and all-reduce of `step`'s 1: the [B, d] input rows;
          2. `train_shard_forward_only` on every local model: the encoder, the scorer over the own rows, this shard's loss double;
          3. all-gather of the G loss doubles;
          4. only with `want_predictions` on a sampled batch: one all-reduce of [B, L] (one non-zero addend per element: exact).

        Returns `(loss, pred or None, h or None)`.  loss: the doubles added in rank order times 1 / (B L) (sampled) or 1 / (B num_ent)
        (1-vs-all), rounded to float32, a 1-element device tensor (rank 0's in the in-process form, as `step`).  Sampled predictions
        are the full [B, L].  1-vs-all predictions are NOT exchanged (nothing logit-sized moves): each rank gets its own [B, n_local]
        block, the in-process form the list of blocks in rank order.  h [B, d] is the same on every rank.  In the deferred-rows mode a
        sampled batch is scored against every row as of the current update and no row is brought current in the table."""
        ms = self.local
        lv = batch.get("lookup_values", None)
        sampled = "e2_multi" in batch and lv is not None and np.ndim(lv) == 2 and np.shape(lv)[1] > 0      # (data.py: [B, 0] means 1-vs-all)
        if not sampled and ("lab_indptr" not in batch or "e2_multi" in batch):
            raise ValueError("EntityShardedTrainer.forward: a 1-vs-all batch with sparse labels (lab_indptr, lab_idx [, lab_row]) or a sampled "
                             "batch (lookup_values, e2_multi [B, L]); dense e2_multi [B, num_ent] is not served")
        if not sampled and any(m.train_rows_deferred == 1 for m in ms):
            raise ValueError("EntityShardedTrainer.forward: the models are in the deferred-rows mode, which serves sampled batches only (1-vs-all "
                             "scores read every row)")
        B = len(batch["e1"])
        rows = self._exchange([m.train_shard_gather(batch["e1"]) for m in ms], reduce=True)                      # 1
        outs = [m.train_shard_forward_only(batch, r, want_predictions, want_h) for m, r in zip(ms, rows)]         # 2
        ls_all = self._exchange([o[0] for o in outs])                                                             # 3
        n_labels = float(B) * float(np.shape(lv)[1] if sampled else ms[0].num_ent)
        total = ls_all[0].reshape(-1)
        acc = total[0:1].clone()
        for g in range(1, self.world):      # rank order
            acc += total[g:g + 1]
        loss = (acc * (1.0 / n_labels)).to(torch.float32)
        pred = None
        if want_predictions and sampled:
            pred = self._exchange([o[1] for o in outs], reduce=True)[0]                                           # 4
        elif want_predictions:
            pred = [o[1] for o in outs] if self._in_process else outs[0][1]
        return loss, pred, outs[0][2]

    def sync_rows(self):
        """Deferred rows: every owned row of every local model current (`ConvE.train_sync_rows`); nothing to do with the mode off.  A
        rank's registered ent_emb / pred_bias tensors are current only behind this, or behind one of the calls that sync by themselves."""
        for m in self.local:
            m.train_sync_rows()
        return self
