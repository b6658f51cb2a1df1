"""Shared by tests/test_gpu_train_split.py and tests/test_gpu_train_parallel.py: the float64 oracle of an update made from several
micro-batch gradients (oracle/coper_train_oracle.py through train_step / forward_train, dropout_keep and AMSGrad), and the step-0
bounds of tests/test_gpu_train.py::_train_step_case as one function."""
import numpy as np

from coper_amd import data as cdata
from tests.test_gpu_train import _CASES, _rel_err

SEED = 5
CLIP = 5.0


def md_for(name, **over):
    md = dict(cdata._COMMON)
    md.update(_CASES[name])
    md.update(batch_norm_train_stats=True, batch_norm_momentum=0.9, hidden_dropout=0.3, output_dropout=0.2, label_smoothing_epsilon=0.1,
              learning_rate=0.003)
    md.update(over)
    return md


def batch(md, form, B, L, seed):
    """tests/test_gpu_train.py::_batch (e1 and rel over all ids) in one of the three label forms: "sampled"; "dense" (the same labels
    scattered into e2_multi [B, |E|], as _train_step_case does); "csr" (those rows as id lists, one table row per sample)."""
    from tests.test_gpu_train import _batch
    b = _batch(md, B, L, seed)
    if form == "sampled":
        return b
    dense = np.zeros((B, md["num_ent"]), np.float32)
    np.put_along_axis(dense, b["lookup_values"].astype(np.int64), b["e2_multi"], axis=1)
    if form == "dense":
        return dict(e1=b["e1"], rel=b["rel"], e2_multi=dense, lookup_values=np.zeros((B, 0), np.int32))
    rows = [np.nonzero(dense[i])[0].astype(np.int64) for i in range(B)]
    return dict(e1=b["e1"], rel=b["rel"], lab_indptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                lab_idx=np.concatenate(rows), lab_row=np.arange(B, dtype=np.int64))


def oracle_batch(md, batch):
    """A model batch (any of the three label forms) as the oracle's dict."""
    if "e2_multi" not in batch:
        E = md["num_ent"]
        ip, ix = np.asarray(batch["lab_indptr"]), np.asarray(batch["lab_idx"])
        rows = batch.get("lab_row", None)
        rows = np.arange(len(batch["e1"])) if rows is None else np.asarray(rows)
        dense = np.zeros((len(rows), E), np.float32)
        for b, r in enumerate(rows):
            dense[b, ix[ip[r]:ip[r + 1]]] = 1.0
        return dict(e1=np.asarray(batch["e1"]), rel=np.asarray(batch["rel"]), lookup=None, labels=dense)
    lv = batch.get("lookup_values", None)
    one_vs_all = lv is None or np.shape(lv)[1] == 0
    return dict(e1=np.asarray(batch["e1"]), rel=np.asarray(batch["rel"]), lookup=None if one_vs_all else np.asarray(lv),
                labels=np.asarray(batch["e2_multi"]))


class _NoUpdate(object):
    """An optimizer for coper_train_oracle.train_step that leaves the variables alone: the call is then the oracle's BACKWARD --
    loss, gradients, the BN moving statistics moved -- with the masks of dropout counter `step`."""

    def step(self, params, grads):
        return np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values()))


def oracle_backward(ref, md, batch, seed, step):
    """-> (loss, grads); ref's moving statistics are updated, nothing else."""
    from oracle import coper_train_oracle as T
    loss, grads, _ = T.train_step(ref, md, oracle_batch(md, batch), _NoUpdate(), seed=seed, step=step, momentum=md["batch_norm_momentum"])
    return loss, grads


def oracle_update(ref, opt, grads_list):
    """The mean of the gradients in grads_list through ONE AMSGrad.step on ref -> (mean gradients, their global norm)."""
    mean = {k: sum(g[k] for g in grads_list) / float(len(grads_list)) for k in grads_list[0]}
    tr = {k: np.asarray(ref[k], np.float64) for k in mean}
    gn = opt.step(tr, mean)
    for k in mean:
        ref[k] = tr[k]
    return mean, gn


def new_oracle(md, p0, clip=CLIP):
    from oracle import coper_train_oracle as T
    ref = {k: np.array(v, np.float64) for k, v in p0.items()}
    return ref, T.AMSGrad(T.trainable_names(md), ref, lr=md["learning_rate"], clip=clip)


def check_grads(got, want, gn_o, what=""):
    """Gradients against the oracle's by the step-0 bound (2e-4 by _rel_err) -> {leaf: max |difference|}"""
    dg = {}
    for leaf, w in want.items():
        g = np.asarray(got[leaf]).reshape(w.shape)
        err = _rel_err(g, w, 1e-3 * gn_o)
        print("  %s %-40s rel err %.3g" % (what, leaf, err))
        assert err < 2e-4, (what, leaf, err)
        dg[leaf] = np.abs(g - w).max()
    return dg


def check_variables(md, tensors, ref, dg, what="", skip_stats=False):
    """The variables against the oracle's by _train_step_case's step-0 formula.  tensors: {leaf: host array}."""
    train_stats = md["batch_norm_train_stats"]
    for leaf, want in ref.items():
        if train_stats and leaf == "conv1_bias":      # (exact gradient 0 under batch statistics: nothing to compare, as there)
            continue
        if skip_stats and leaf.endswith(("moving_mean", "moving_variance")):
            continue
        got = np.asarray(tensors[leaf]).reshape(np.shape(want))
        lr_t = md["learning_rate"] * 0.32
        tol = 2e-5 + 1e-5 * np.abs(want).max() + 2.0 * lr_t * 0.1 * dg.get(leaf, 0.0) / 1e-8
        if train_stats and leaf == "Conv1BN/moving_mean" and "conv1_bias" in ref:
            bias = np.asarray(tensors["conv1_bias"]).reshape(-1)
            tol += np.abs(bias - np.reshape(ref["conv1_bias"], -1)).max()
        diff = np.abs(got - want).max()
        print("  %s %-40s |diff| %.3g tol %.3g" % (what, leaf, diff, tol))
        assert diff < tol, (what, leaf, diff, tol)


def flat_slices(flat, layout):
    """The flat gradient vector (host array) cut into {leaf: array}."""
    return {leaf: flat[off:off + n] for leaf, (off, n) in layout.items()}
