"""GPU tests that a training call's results do not depend on the handle's earlier calls (include/coper_hip.h,
coper_train_config.deterministic: "the same bits ... on another handle").

tests/train_history_common.py has the harness and the op notation.  In the deterministic modes a call on a handle with a history must
leave the bits of the same call on a freshly created handle loaded with the first one's variables, BN statistics, slots, powers and
step counter; the default mode has no bit promise and is held to the float64 oracle after every step of a history.

Shapes are the smallest at which a capacity word of TrainState (coper_train.hip) moves; models are tests/test_gpu_train.py::_CASES
through D._md: E = 211, d = 40 (cpg_wide: E = 700, d = 200).  one_vs_all_chunk = 128: a CSR step at E = 211 has two chunks.

  H1        capB / capL and the workspaces sized from them in all three label forms, Sd, det_slab, the plane sets, the split step's
            pending gradients, the inference caches between steps, wmax_valid / wmax_cur, exp_cache
  H1-first  each label form as the first call a handle ever sees (capL = 1 after a 1-vs-all first call)
  H2        the split-K pool and multi-tile GEMM planes (d = 200), B across one 128-row tile
  H3        ord_cap (one and three sort tiles), Sd appearing with the switch off, the switch itself
  H4        rows_cap by rows_grow (with a list owed its re-zero) and by rows_grow_keep, rows_prev, the claim bits, the mode switch
  H5        sh_B / sh_cap of a sharded state in both label forms
  H6        the default mode's atomics-and-zeroing routes over the same shapes"""
import numpy as np
import pytest

from tests import test_gpu_train_deterministic as D
from tests import train_history_common as HC
from tests.test_train_order_abi import kernel_constants

pytestmark = pytest.mark.gpu

TILE = kernel_constants()["COPER_ORDER_SORT_TILE"]

_H1_STEPS = [("S", 16, 37), ("D", 48), ("S", 48, 37),      # a 1-vs-all call grows B, then the first sampled call at that B with L == capL
             ("S", 70, 9), ("S", 16, 60), ("S", 70, 60),   # B L above every earlier product while neither maximum grows
             ("C", 80)]                                    # a CSR call grows B over two chunks
_H1_TAIL = [("S", 1, 1), ("D", 16)]
H1 = _H1_STEPS + [("F", "sampled", 5, 37), ("F", "dense", 80, 0), ("F", "csr", 5, 0), ("BA", "sampled", 33, 21), ("BEA", "dense", 96, 0),
                  ("EVAL",)] + _H1_TAIL
H2 = [("S", 16, 9), ("S", 130, 60), ("D", 48), ("C", 130), ("S", 16, 9)]
H3 = [("S", 16, 37), ("ORDER", False), ("S", 48, 37), ("ORDER", True), ("S", 48, 37), ("S", 77, 2 * TILE // 77 + 8), ("S", 16, 9), ("C", 48),
      ("S", 70, 60)]
H4 = [("S", 16, 37), ("ROWS", 48, 37, False, 1.0),         # rows_grow while the list of the step before is owed its re-zero
      ("S", 5, 9), ("SYNC",), ("REFUSED", "csr", 48), ("DEFER", False), ("S", 70, 60), ("DEFER", True), ("ROWS", 70, 60, True, 0.5), ("S", 16, 9)]
# the row lists sized by imports alone: rows_grow_keep from a list of 2 entries (on the fresh handle: from none)
H4_KEEP = [("S", 1, 1), ("IMPORT", 40, 90, 0.5), ("S", 16, 9), ("IMPORT", 150, 211, 1.0), ("S", 5, 9)]
H5 = [("C", 16), ("S", 48, 37), ("C", 80), ("S", 80, 37), ("S", 16, 60), ("C", 16)]


@pytest.mark.parametrize("name", ["cpg_linear", "lookup", "cpg_linear_concat", "cpg_conv_mlp"])
def test_h1_deterministic(name):
    """The four models own different workspaces: generated dense planes, the looked-up layer's partial sums in dx, xc / dxc, Kt / Kbv."""
    HC.run_checkpointed(D._md(name), HC.mode_of(), H1)


@pytest.mark.parametrize("first", [("S", 16, 37), ("D", 16), ("C", 16)], ids=["sampled", "dense", "csr"])
def test_h1_each_label_form_first(first):
    HC.run_checkpointed(D._md("cpg_linear"), HC.mode_of(), [first, ("S", 48, 37), ("D", 48), ("C", 48)])


def test_h2_deterministic_wide():
    HC.run_checkpointed(D._md("cpg_wide"), HC.mode_of(), H2)


def test_h3_ordered():
    HC.run_checkpointed(D._md("cpg_linear"), HC.mode_of(ordered=True), H3)


@pytest.mark.parametrize("ops", [H4, H4_KEEP], ids=["h4", "h4_keep"])
def test_h4_ordered_deferred_checkpointed(ops):
    HC.run_checkpointed(D._md("cpg_linear"), HC.mode_of(ordered=True, deferred=True), ops)


def test_h3_ordered_end_to_end():
    """No deferred rows: nothing a read could perturb, so the unread history and the chain of fresh handles agree to the bit."""
    lh, lf, end_h, end_f = HC.run_end_to_end(D._md("cpg_linear"), HC.mode_of(ordered=True), H3)
    _same_losses(lh, lf, H3)
    HC.compare(end_h, end_f, "H3 end to end")


def _same_losses(la, lb, ops):
    for k, (a, b) in enumerate(zip(la, lb)):
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes()), (k, ops[k], a, b)


def test_h4_ordered_deferred_end_to_end():
    """The unread history against the chain of fresh handles, whose every state read brings all rows current.  That is the same
    arithmetic as long as no row is more than ONE update behind when it is brought current (a single zero-gradient update, whoever
    applies it) -- H4's batches at E = 211 name nearly every row, and the host-side count below holds that.  Past one update the
    header promises rounding only: test_h4_gaps_between_twins covers that side to the bit."""
    md, mode = D._md("cpg_linear"), HC.mode_of(ordered=True, deferred=True)
    assert HC.max_row_gap(md, mode, H4) == 1
    lh, lf, end_h, end_f = HC.run_end_to_end(md, mode, H4)
    _same_losses(lh, lf, H4)
    HC.compare(end_h, end_f, "H4 end to end")


def test_h4_gaps_between_twins():
    """H4 at E = 20,011, where rows stay several updates behind: a fresh twin against one whose row lists, sort workspace and slabs an
    earlier B = 300, L = 64 step and a rows group with imports grew; nothing is read between the ops."""
    from tests.test_gpu_train_ordered import _small_md
    md, mode = _small_md(20011), HC.mode_of(ordered=True, deferred=True)
    assert HC.max_row_gap(md, mode, H4) >= 3
    la, lb, end_a, end_b = HC.run_twins(md, mode, [("S", 300, 64), ("ROWS", 70, 60, True, 0.5)], H4)
    _same_losses(la, lb, H4)
    HC.compare(end_a, end_b, "H4 with gaps, twins")


def test_h5_sharded():
    HC.run_sharded(D._md("cpg_linear"), [(0, 100), (100, 211)], H5)


@pytest.mark.parametrize("name,ops", [("cpg_linear", _H1_STEPS + _H1_TAIL), ("cpg_wide", H2)], ids=["h1_steps", "h2"])
def test_h6_default_mode_against_the_oracle(name, ops):
    """The bounds of tests/test_gpu_train.py::test_train_batch_shape_changes_between_steps, unchanged: loss 2e-5, gradients 2e-4 by
    _rel_err with a floor of 1e-3 of the norm, norm 1e-4; the oracle restarts from the device's variables before each step and is fed
    a CSR batch as its densified labels."""
    from oracle import coper_train_oracle as T
    from tests.split_common import oracle_batch
    md = D._md(name)
    with HC.LiveBytes():
        p0 = HC.p0_for(md)
        m = HC.new_handle(md, (p0, None), HC.mode_of(deterministic=False))
        try:
            ref = {k: v.numpy().astype(np.float64) for k, v in p0.items()}
            opt = T.AMSGrad(T.trainable_names(md), ref, lr=md["learning_rate"], clip=5.0)
            for step, op in enumerate(ops):
                for k in ref:
                    ref[k] = m._tensors[k].cpu().numpy().reshape(np.shape(ref[k])).astype(np.float64)
                batch = HC.op_batch(md, op, step)
                loss_o, grads_o, gn_o = T.train_step(ref, md, oracle_batch(md, batch), opt, seed=HC.SEED, step=step,
                                                     momentum=md["batch_norm_momentum"])
                loss = float(m.train_step(batch).cpu()[0])
                print("step %d %r loss %.9g oracle %.9g" % (step, op, loss, loss_o))
                assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (step, op, loss, loss_o)
                for leaf in T.trainable_names(md):
                    g, gn = m.train_grad(leaf)
                    err = D._rel_err(g.cpu().numpy().reshape(grads_o[leaf].shape), grads_o[leaf], 1e-3 * gn_o)
                    print("  %-40s rel err %.3g" % (leaf, err))
                    assert err < 2e-4, (step, op, leaf, err)
                print("  norm %.9g oracle %.9g" % (gn, gn_o))
                assert abs(gn - gn_o) < 1e-4 * gn_o, (step, op, gn, gn_o)
        finally:
            m.close()


def test_the_comparison_sees_a_stale_state():
    """The harness's own check: a fresh handle loaded with the state from one op EARLIER than the history handle's fails the
    comparison; loaded with the right state it passes."""
    md = D._md("cpg_linear")
    ops = [("S", 16, 37), ("S", 48, 37)]
    with HC.LiveBytes():
        mode = HC.mode_of()
        H = HC.new_handle(md, (HC.p0_for(md), None), mode)
        try:
            states = []
            for k, op in enumerate(ops):
                states.append(HC._save(H))
                got_h = HC.run_op(H, md, op, k, mode)
            got = []
            for state in states:
                F = HC.new_handle(md, state, mode)
                try:
                    got.append(HC.run_op(F, md, ops[1], 1, mode))
                finally:
                    F.close()
        finally:
            H.close()
        with pytest.raises(AssertionError):
            HC.compare(got_h, got[0], "the state of one op earlier")
        HC.compare(got_h, got[1], "the state in front of the op")
