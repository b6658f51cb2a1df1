"""GPU tests of 1-vs-all training from sparse labels (include/coper_hip.h: coper_train_step_csr / coper_train_forward_csr): the id
lists a dense e2_multi [B, |E|] is built from, the scorer walked in chunks of entity columns (coper_train_config.one_vs_all_chunk).

Bounds: the step-0 ("tight") bounds of tests/test_gpu_train.py::_train_step_case, restated in `_check_against_oracle`; the float64
oracle (oracle/coper_train_oracle.py) receives the densified labels and restarts from the device's variables before every step.
Model dimensions are those of that file's _CASES."""
import numpy as np
import pytest
import torch

from coper_amd import data as cdata

pytestmark = pytest.mark.gpu

_DIMS = {
    "cpg_linear": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                       context_rel_conv=None, context_rel_out=[]),
    "plain": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=40, emb_h=10, emb_w=4, conv_num_channels=8,
                  context_rel_conv=None, context_rel_out=None),
    "lookup": dict(num_ent=211, num_rel=6, ent_emb_size=40, rel_emb_size=1, emb_h=10, emb_w=4, conv_num_channels=8,
                   context_rel_conv=None, context_rel_out=[], do_parameter_lookup=True),
    "cpg_wide": dict(num_ent=700, num_rel=6, ent_emb_size=200, rel_emb_size=8, emb_h=10, emb_w=20, conv_num_channels=32,
                     context_rel_conv=None, context_rel_out=[]),
    "cpg_linear_e20k": dict(num_ent=20011, num_rel=6, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=8,
                            context_rel_conv=None, context_rel_out=[]),
    # past the dense-label call's 512 MiB cap at B = 129 (129 * 1,048,583 * 4 = 541 MB): d = 12 as 3 x 4, three channels, a 2 x 2 filter
    "cpg_linear_e1m": dict(num_ent=1048583, num_rel=6, ent_emb_size=12, rel_emb_size=8, emb_h=3, emb_w=4, conv_num_channels=3,
                           conv_filter_height=2, conv_filter_width=2, context_rel_conv=None, context_rel_out=[]),
}
_SEED = 5


def _md(name):
    md = dict(cdata._COMMON)
    md.update(_DIMS[name])
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=0.003)
    return md


def _model(md, p0, chunk=0):
    from coper_amd.models import ConvE
    m = ConvE(md, device="cuda:0")
    m.load_parameters({k: torch.as_tensor(np.array(v, np.float32)) for k, v in p0.items()})
    m.train_init(seed=_SEED, one_vs_all_chunk=chunk)
    return m


def _table(rows):
    """rows: lists of entity ids (made ascending) -> (lab_indptr, lab_idx)"""
    rows = [np.unique(np.asarray(r, np.int64)) for r in rows]
    return (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
            np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64))


def _densify(indptr, idx, lab_row, E):
    out = np.zeros((len(lab_row), E), np.float32)
    for b, r in enumerate(lab_row):
        out[b, idx[indptr[r]:indptr[r + 1]]] = 1.0
    return out


def _random_rows(rng, n, E, p=0.05):
    return [np.nonzero(rng.random(E) < p)[0] for _ in range(n)]


def _csr_batch(e1, rel, indptr, idx, lab_row=None):
    b = dict(e1=e1, rel=rel, lab_indptr=indptr, lab_idx=idx)
    if lab_row is not None:
        b["lab_row"] = np.asarray(lab_row, np.int64)
    return b


def _dense_batch(e1, rel, dense):
    return dict(e1=e1, rel=rel, e2_multi=dense, lookup_values=np.zeros((len(e1), 0), np.int32))


def _grads(m, leaves):
    out, gn = {}, None
    for leaf in leaves:
        g, gn = m.train_grad(leaf)
        out[leaf] = g.cpu().numpy()
    return out, gn


def _adjacent_f32(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or np.nextafter(a, b) == b


def _rel_err(a, b, floor):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor)


def _check_against_oracle(name, chunk, B, steps, make_labels):
    """`make_labels(rng, E, B, step)` -> (lab_indptr, lab_idx, lab_row).  Every step is held to the step-0 bounds of
    tests/test_gpu_train.py::_train_step_case: the oracle is restarted from the device's variables before it."""
    from oracle import coper_train_oracle as T
    md = _md(name)
    E, R = md["num_ent"], md["num_rel"]
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = _model(md, p0, chunk)
    ref = {k: np.array(v, np.float64) for k, v in p0.items()}
    opt = T.AMSGrad(T.trainable_names(md), ref, lr=md["learning_rate"], clip=5.0)
    train_stats = md["batch_norm_train_stats"]
    for step in range(steps):
        rng = np.random.default_rng(100 + step)
        e1, rel = rng.integers(0, E, B), rng.integers(0, R, B)
        indptr, idx, lab_row = make_labels(rng, E, B, step)
        dense = _densify(indptr, idx, lab_row, E)
        if step > 0:
            for k in ref:
                ref[k] = m._tensors[k].cpu().numpy().reshape(np.shape(ref[k])).astype(np.float64)
        loss_o, grads_o, gn_o = T.train_step(ref, md, dict(e1=e1, rel=rel, lookup=None, labels=dense), opt, seed=_SEED, step=step,
                                             momentum=md["batch_norm_momentum"])
        loss = float(m.train_step(_csr_batch(e1, rel, indptr, idx, lab_row)).cpu()[0])
        print("step %d loss %.9g oracle %.9g" % (step, loss, loss_o))
        assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (step, loss, loss_o)
        dg = {}
        for leaf in T.trainable_names(md):
            g, gn = m.train_grad(leaf)
            g = g.cpu().numpy().reshape(grads_o[leaf].shape)
            err = _rel_err(g, grads_o[leaf], 1e-3 * gn_o)
            print("  %-40s rel err %.3g" % (leaf, err))
            assert err < 2e-4, (step, leaf, err)
            dg[leaf] = np.abs(g - grads_o[leaf]).max()
        print("  norm %.9g oracle %.9g" % (gn, gn_o))
        assert abs(gn - gn_o) < 1e-4 * gn_o
        for leaf, want in ref.items():
            if train_stats and leaf == "conv1_bias":      # (exact gradient 0 under batch statistics: nothing to compare, as there)
                continue
            got = m._tensors[leaf].cpu().numpy().reshape(np.shape(want))
            lr_t = md["learning_rate"] * 0.32
            tol = 2e-5 + 1e-5 * np.abs(want).max() + 2.0 * lr_t * 0.1 * dg.get(leaf, 0.0) / 1e-8
            if train_stats and leaf == "Conv1BN/moving_mean" and "conv1_bias" in ref:
                bias = m._tensors["conv1_bias"].cpu().numpy().reshape(-1)
                tol += np.abs(bias - np.reshape(ref["conv1_bias"], -1)).max()
            assert np.abs(got - want).max() < tol, (step, leaf, np.abs(got - want).max(), tol)
    m.close()


# The gradients that ONE writer per element forms in the default mode at E = 211, B = 48 (coper_train.hip, struct Step), from inputs that
# are ordered themselves -- h, the logits' gradient S (elementwise behind a GEMM; the GEMMs have no float atomics), dh = S E (GEMM) and
# dz (k_tr_fcbn_bwd):
#   pred_bias                  k_tr_col_sum_f32: a thread per column, the 48 rows added in ascending b, stored with `=`
#   FCBN/gamma, FCBN/beta      k_tr_fcbn_bwd: a workgroup per feature, a fixed LDS tree, stored with `=`
#   fc_weights (plain), fc_weights/CPG/Projection0 (cpg_linear)      x^T dz: a GEMM's stores (tg_matmul / tg_gemm_nt, K = B = 48)
#   fc_bias/CPG/Projection0    k_tr_wsum_rows_add<false>: one atomic per element and 64-row stretch onto the zeroed gradient; B = 48 is
#                              ONE stretch, so 0 + a
# and those that several writers add to in an order that changes from run to run -- held to the float64 oracle instead:
#   ent_emb                    k_tr_conv_bwd<false> adds the e1 rows by float atomics onto the GEMM's dE (e1 repeats in 48 of 211)
#   fc_bias (plain)            k_tr_fc_post_bwd<false>: 48 workgroups' float atomics per element; (lookup) k_tr_lookup_post_bwd<false>
#   fc_weights (lookup)        k_tr_lookup_dW adds in the grouping's arrival order
#   Conv1BN/gamma, /beta       k_tr_bn1_bwd_sums: double atomics; k_tr_bn1_bwd_apply also forms dx from those sums, so everything
#   conv1_weights, conv1_bias, rel_emb      behind the Conv1BN backward inherits their last bits (and is added by float atomics itself)
# What the forward pass reads of unordered sums are the BN batch statistics: double atomics over float addends (k_tr_col_sums<false>)
# rounded ONCE to float32 by k_tr_bn_finish (mean, 1 / std, the moving statistics).  Two orders of a double sum differ by a few 2^-53;
# such a difference moves one of the ~100 float32 roundings of a step only if it straddles a rounding boundary, odds of 1e-7: h, the
# logits and the moving statistics are asserted bit-equal too.
_ORDERED = {
    "cpg_linear": ("pred_bias", "FCBN/gamma", "FCBN/beta", "fc_weights/CPG/Projection0", "fc_bias/CPG/Projection0"),
    "plain": ("pred_bias", "FCBN/gamma", "FCBN/beta", "fc_weights"),
    "lookup": ("pred_bias", "FCBN/gamma", "FCBN/beta"),
}
_CLIP = 5.0      # train_init's clip_norm


@pytest.mark.parametrize("name", ["cpg_linear", "plain", "lookup"])
def test_csr_step_is_the_dense_step_with_one_chunk(name):
    """E = 211 is one chunk: every launch but the loss kernel is the dense-label call's.  Three handles from the same parameters, two fed
    dense labels and one the CSR of the same labels.  The gradients of _ORDERED (one writer per element: the comment above cites the
    kernels) are bit-identical on the three handles, and so are the variables their update moves while the clip is idle (asserted),
    and the BN moving statistics.  Every other gradient of the CSR handle, and its norm, is held to the float64 oracle of the same
    step within _check_against_oracle's bounds.  The loss is summed by double atomics in any order: equal or an adjacent float32.
    `plain` passes a per-batch CSR without lab_row.

    Until this test named the ordered leaves it took whatever the two dense handles agreed on as ordered, and failed 4 runs of 12:
    `assert np.array_equal(gc[k], ga[k])` at k = 'ent_emb' (one or two ulp, 1.2e-10) -- the two dense handles' float atomics had
    happened to land in the same order and the CSR handle's had not."""
    from oracle import coper_train_oracle as T
    md = _md(name)
    E, R, B = md["num_ent"], md["num_rel"], 48
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    da, db, cs = _model(md, p0), _model(md, p0), _model(md, p0)
    leaves = T.trainable_names(md)
    ordered = _ORDERED[name]
    assert "pred_bias" in ordered and set(ordered) <= set(leaves)
    ref = {k: np.array(v, np.float64) for k, v in p0.items()}
    opt = T.AMSGrad(leaves, ref, lr=md["learning_rate"], clip=_CLIP)
    for step in range(2):
        rng = np.random.default_rng(300 + step)
        e1, rel = rng.integers(0, E, B), rng.integers(0, R, B)
        if name == "plain":
            indptr, idx = _table(_random_rows(rng, B, E))
            lab_row, rows = None, np.arange(B)
        else:
            indptr, idx = _table(_random_rows(rng, 30, E))
            lab_row = rows = rng.integers(0, 30, B)
        dense = _densify(indptr, idx, rows, E)
        csr_batch = _csr_batch(e1, rel, indptr, idx, lab_row)
        if step == 0:
            # the train-mode forward without the update, while the three handles still hold the same variables: the dense call's h and
            # logits bit for bit on all three (the comment above _ORDERED), and nothing written
            before = {k: v.clone() for k, v in cs._tensors.items()}
            loss_fd, pred_d, h_d = da.train_forward(_dense_batch(e1, rel, dense), want_predictions=True, want_h=True)
            _, pred_b, h_b = db.train_forward(_dense_batch(e1, rel, dense), want_predictions=True, want_h=True)
            loss_fc, pred_c, h_c = cs.train_forward(csr_batch, want_predictions=True, want_h=True)
            assert tuple(pred_c.shape) == (B, E)
            assert torch.equal(h_b, h_d) and torch.equal(pred_b, pred_d)
            assert torch.equal(h_c, h_d) and torch.equal(pred_c, pred_d)
            assert _adjacent_f32(loss_fc.cpu()[0].item(), loss_fd.cpu()[0].item())
            assert all(torch.equal(before[k], cs._tensors[k]) for k in before)
        # the float64 oracle of this step, from the variables the three handles hold in front of it
        for k in ref:
            ref[k] = cs._tensors[k].cpu().numpy().reshape(np.shape(ref[k])).astype(np.float64)
        loss_o, grads_o, gn_o = T.train_step(ref, md, dict(e1=e1, rel=rel, lookup=None, labels=dense), opt, seed=_SEED, step=step,
                                             momentum=md["batch_norm_momentum"])
        la = float(da.train_step(_dense_batch(e1, rel, dense)).cpu()[0])
        lb = float(db.train_step(_dense_batch(e1, rel, dense)).cpu()[0])
        lc = float(cs.train_step(csr_batch).cpu()[0])
        if step == 0:
            assert _adjacent_f32(lc, loss_fc.cpu()[0].item())       # (the forward drew the masks of this step)
        assert _adjacent_f32(la, lb) and _adjacent_f32(lc, la), (la, lb, lc)
        assert abs(lc - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (step, lc, loss_o)
        ga, na = _grads(da, leaves)
        gb, nb = _grads(db, leaves)
        gc, nc = _grads(cs, leaves)
        for k in ordered:
            assert np.array_equal(ga[k], gb[k]), (step, k, np.abs(ga[k] - gb[k]).max())
            assert np.array_equal(gc[k], ga[k]), (step, k, np.abs(gc[k] - ga[k]).max())
        for k in leaves:      # (the ordered ones too: bit-equal to each other says nothing about their value)
            err = _rel_err(gc[k].reshape(grads_o[k].shape), grads_o[k], 1e-3 * gn_o)
            print("step %d  %-40s rel err %.3g%s" % (step, k, err, "  (ordered)" if k in ordered else ""))
            assert err < 2e-4, (step, k, err)
        # the norm is a double summed by atomics over all leaves: against the oracle, on each handle
        print("step %d  norm %.17g %.17g %.17g oracle %.17g" % (step, na, nb, nc, gn_o))
        for n in (na, nb, nc):
            assert abs(n - gn_o) < 1e-4 * gn_o, (step, n, gn_o)
            assert n < _CLIP      # the clip is idle: the update's factor clip / max(norm, clip) is exactly 1
        # the variables after the step: an ordered gradient through AMSGrad with the factor 1, and the BN moving statistics (no
        # gradient: the forward's batch statistics decide), are the same computation on the three handles
        for k in da._tensors:
            if k in ordered or k not in leaves:
                assert torch.equal(da._tensors[k], db._tensors[k]), (step, k)
                assert torch.equal(cs._tensors[k], da._tensors[k]), (step, k)
        if step == 0:
            # the embedding rows of the batch's e1 are added by float atomics: the three trajectories part there.  The second step
            # starts all three from the first handle's state again (variables, optimizer slots), registered anew on each
            slots, powers = da.optimizer_state()
            for m in (da, db, cs):
                m.load_parameters({k: v.clone() for k, v in da._tensors.items()})
                m.load_optimizer_state(slots, powers)
    for m in (da, db, cs):
        m.close()


def _edge_labels(chunk):
    def make(rng, E, B, step):
        rows = _random_rows(rng, 20, E)
        rows[0] = [0, chunk - 1, chunk, E - 1]      # both sides of a chunk edge, the table's first and last column
        rows[1] = []                                # an empty row
        rows[2] = np.arange(E)                      # every entity positive
        indptr, idx = _table(rows)
        lab_row = rng.integers(0, 20, B)
        lab_row[:8] = [7, 3, 3, 0, 1, 2, 19, 0]     # a repeated row, rows out of order
        return indptr, idx, lab_row
    return make


@pytest.mark.parametrize("name,chunk", [("cpg_linear", 128), ("plain", 128), ("cpg_wide", 256)])
def test_chunked_csr_step_matches_oracle(name, chunk):
    """E = 211 as chunks of 128 + 83 (the grain is 128), E = 700 at d = 200 as 256 + 256 + 188: all leaves, loss, norm and variables
    against the float64 oracle over two steps."""
    _check_against_oracle(name, chunk, B=48, steps=2, make_labels=_edge_labels(chunk))


def test_long_row_across_lds_stretches_matches_oracle():
    """E = 20,011 in chunks of 8,192 (8,192 + 8,192 + 3,627; a chunk is four stretches of the loss kernel's bitmask): a row with 5,000
    positives spread over all three chunks, an empty row, positives on both sides of every chunk edge and at the last column."""
    def make(rng, E, B, step):
        rows = _random_rows(rng, B, E, p=0.001)
        rows[0] = rng.choice(E, 5000, replace=False)
        assert all(((rows[0] >= lo) & (rows[0] < hi)).sum() > 500 for lo, hi in ((0, 8192), (8192, 16384), (16384, E)))
        rows[1] = []
        rows[2] = [8191, 8192, 16383, 16384, 20010]
        indptr, idx = _table(rows)
        return indptr, idx, rng.permutation(B)
    _check_against_oracle("cpg_linear_e20k", 8192, B=24, steps=1, make_labels=make)


def test_csr_step_trains_past_the_dense_label_cap():
    """E = 1,048,583 at B = 129: B * E * 4 = 541 MB.  The dense-label call still refuses it with its 512 MiB message; the CSR call runs
    it as four chunks of 262,144 columns and one of 7.  The float64 torch oracle is not run at this size (5.7 s and 9.1 GB on the host):
    h comes from coper_train_forward_csr (the step that follows draws the same masks), and loss, d(pred_bias) and d(ent_emb) = ds^T h
    are formed from it in NumPy float64, chunked over columns.  The ent_emb rows of the batch's e1 also carry the conv's gradient and
    are left out.  Bounds: _train_step_case's, the gradients without its floor (the oracle's global norm is not known here)."""
    from coper_amd._lib import CoperError
    md = _md("cpg_linear_e1m")
    E, R, B, d, chunk = md["num_ent"], md["num_rel"], 129, md["ent_emb_size"], 262144
    assert B * E * 4 > 512 * 1024 * 1024
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    m = _model(md, p0, chunk)
    rng = np.random.default_rng(9)
    e1, rel = rng.integers(0, E, B), rng.integers(0, R, B)
    with pytest.raises(CoperError, match="512 MiB"):
        m.train_step(_dense_batch(e1, rel, torch.empty((B, E), dtype=torch.float32, device="cuda:0")))
    torch.cuda.empty_cache()
    edges = [0, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, 3 * chunk, 4 * chunk - 1, 4 * chunk, E - 1]
    rows = [np.concatenate([rng.choice(edges, 2, replace=False), rng.integers(0, E, 3)]) for _ in range(B)]
    rows = [np.unique(r) if len(np.unique(r)) == 5 else np.array([1, 2, 3, chunk, E - 1]) for r in rows]      # five positives per row
    indptr, idx = _table(rows)
    lab_row = rng.permutation(B)
    batch = _csr_batch(e1, rel, indptr, idx, lab_row)
    ent, bias = np.asarray(p0["ent_emb"], np.float64).reshape(E, d), np.asarray(p0["pred_bias"], np.float64).reshape(E)
    loss_f, _, hv = m.train_forward(batch, want_h=True)
    h = hv.cpu().numpy().astype(np.float64)
    loss = float(m.train_step(batch).cpu()[0])
    g_bias = m.train_grad("pred_bias")[0].cpu().numpy()
    g_ent = m.train_grad("ent_emb")[0].cpu().numpy().reshape(E, d)
    torch.cuda.synchronize()
    # the reference, a stretch of columns at a time
    eps, total = md["label_smoothing_epsilon"], 0.0
    dbias, dE = np.empty(E), np.empty((E, d))
    pos_b = np.repeat(np.arange(B), 5)
    pos_c = np.concatenate([idx[indptr[r]:indptr[r + 1]] for r in lab_row])
    for c0 in range(0, E, 131072):
        c1 = min(E, c0 + 131072)
        s = h @ ent[c0:c1].T + bias[c0:c1]
        t = np.full(s.shape, 1.0 / E)
        sel = (pos_c >= c0) & (pos_c < c1)
        t[pos_b[sel], pos_c[sel] - c0] += 1.0 - eps
        ex = np.exp(-np.abs(s))
        total += float((np.maximum(s, 0.0) - s * t + np.log1p(ex)).sum())
        ds = (np.where(s >= 0, 1.0, ex) / (1.0 + ex) - t) / (float(B) * E)
        dbias[c0:c1] = ds.sum(0)
        dE[c0:c1] = ds.T @ h
    loss_o = total / (float(B) * E)
    print("loss %.9g forward %.9g reference %.9g" % (loss, float(loss_f.cpu()[0]), loss_o))
    assert abs(loss - loss_o) < 2e-5 * max(1.0, abs(loss_o)), (loss, loss_o)
    assert abs(float(loss_f.cpu()[0]) - loss_o) < 2e-5 * max(1.0, abs(loss_o))
    err_b = _rel_err(g_bias, dbias, 0.0)
    keep = np.ones(E, bool)
    keep[e1] = False
    err_e = _rel_err(g_ent[keep], dE[keep], 0.0)
    print("pred_bias rel err %.3g, ent_emb rel err %.3g" % (err_b, err_e))
    assert err_b < 2e-4 and err_e < 2e-4, (err_b, err_e)
    m.close()


def test_bad_label_ids_are_treated_as_absent():
    """A lab_idx entry of -1, one equal to num_ent, and lab_row entries outside the table: the loss and the pred_bias gradient of the
    batch without those entries (the bad rows as empty rows), and no error on the stream.  Two chunks, so that the ids past the table
    meet the last chunk's ragged end."""
    md = _md("cpg_linear")
    E, R, B = md["num_ent"], md["num_rel"], 48
    p0 = cdata.synthetic_params(md, seed=21, ent_std=0.1)
    rng = np.random.default_rng(17)
    e1, rel = rng.integers(0, E, B), rng.integers(0, R, B)
    rows = _random_rows(rng, 12, E)
    lab_row = rng.integers(0, 12, B)
    clean_rows = rows + [[]]
    clean_lab_row = lab_row.copy()
    clean_lab_row[[4, 9, 20]] = 12                  # the empty row
    bad_lab_row = lab_row.copy()
    bad_lab_row[4], bad_lab_row[9] = 13, -2         # outside the table of 13 rows
    bad_lab_row[20] = 12                            # (there the row whose only entry is num_ent)
    indptr, idx = _table(clean_rows)
    bad_idx = np.concatenate([[-1], idx[indptr[0]:indptr[3]], [E], idx[indptr[3]:], [E]]).astype(np.int64)      # rows 0, 2 and 12 carry them
    bad_indptr = indptr.copy()
    bad_indptr[1:3] += 1
    bad_indptr[3:] += 2
    bad_indptr[-1] += 1
    assert _densify(indptr, idx, clean_lab_row, E).sum() > 0
    out = []
    for ip, ix, lr in ((indptr, idx, clean_lab_row), (bad_indptr, bad_idx, bad_lab_row)):
        m = _model(md, p0, 128)
        loss = float(m.train_step(_csr_batch(e1, rel, ip, ix, lr)).cpu()[0])
        g = m.train_grad("pred_bias")[0].cpu().numpy()
        torch.cuda.synchronize()
        out.append((loss, g))
        m.close()
    assert _adjacent_f32(out[0][0], out[1][0]), (out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])


def test_one_vs_all_training_from_sparse_labels_through_the_loader():
    """The small graph of tests/test_gpu_train.py::test_one_vs_all_training_through_the_loader with
    `train_dataset(num_labels=None, device=, sparse_labels=True)`: over 200 steps the loss falls and the filtered MRR on the training
    triples ends above what that test asks of the dense route (its start + 0.1)."""
    from coper_amd.data import EvalDataset, OneVsAllTrainDataset, SyntheticKGLoader
    from coper_amd.metrics import ranking_and_hits
    from coper_amd.models import ConvE
    md = cdata.model_descriptors("nations_cpg", ent_emb_size=40, rel_emb_size=40, emb_h=10, emb_w=4, context_rel_conv=None,
                                 context_rel_out=None, conv_num_channels=8, num_ent=60, num_rel=8)
    md.update(use_negative_sampling=False, batch_norm_train_stats=False, hidden_dropout=0.1, output_dropout=0.1,
              label_smoothing_epsilon=0.1, learning_rate=0.003)
    ld = SyntheticKGLoader("nations_plain_like", seed=1, queries=300, md=md)
    ds = ld.train_dataset(None, batch_size=64, num_labels=None, device="cuda:0", sparse_labels=True)
    assert isinstance(ds, OneVsAllTrainDataset) and ds.labels == "csr"
    s = ld.train_samples()
    m = ConvE(md, device="cuda:0").load_parameters(cdata.reference_init_params(md, 3))
    n = np.diff(s["tail_indptr"])
    q = dict(e1=np.repeat(s["e1"], n), rel=np.repeat(s["rel"], n), e2=s["tail_idx"].astype(np.int64),
             filt_indptr=np.concatenate([[0], np.cumsum(np.repeat(n, n))]).astype(np.int64),
             filt_idx=np.concatenate([s["tail_idx"][s["tail_indptr"][i]:s["tail_indptr"][i + 1]] for i in range(len(n)) for _ in range(n[i])]).astype(np.int64))
    mrr0 = ranking_and_hits(m, None, EvalDataset(q, 256, md["num_ent"]), "before")[1]
    sess = m.session()
    it = iter(ds)
    losses = []
    for step in range(200):
        loss, _ = sess.run((m.loss, m.train_op), {m.is_train: True, m.input_iterator_handle: it})
        losses.append(loss)
    mrr1 = ranking_and_hits(m, None, EvalDataset(q, 256, md["num_ent"]), "after")[1]
    print("loss %.4f -> %.4f, MRR %.4f -> %.4f" % (np.mean(losses[:20]), np.mean(losses[-20:]), mrr0, mrr1))
    assert np.mean(losses[-20:]) < 0.7 * np.mean(losses[:20]), (losses[:3], losses[-3:])
    assert mrr1 > mrr0 + 0.1, (mrr0, mrr1)
    m.close()
