"""GPU tests of the training step at the shapes the project ships and benchmarks, against the float64 oracle
(oracle/coper_train_oracle.py in its factored form: the generated weights Wg [B, F, d] and the gathered rows ent_emb[lookup] are
never formed, tests/test_train_oracle.py holds it to the dense form).  Every case is held to the step-0 bounds of
tests/test_gpu_train.py::_train_step_case -- loss 2e-5, gradients 2e-4 of their largest entry, global norm 1e-4, the variables
after the update -- and so is a second step that restarts the oracle from the device's variables.

The training GEMMs choose their kernel and K split from M, N and K alone (tg_use_w128 / tg_split_k in
coper_amd/csrc/train_gemm_bf16.hip).  The small cases of tests/test_gpu_train.py never reach the one-wave-per-128x128-tile kernel
(k_gemm_nt_w128_bf16x3), which carries almost all of a full-size step's FLOPs; each case below names the routes it is here for.
T = x P is the generated dense layer's product ([B] x [r d], K = F), dx = dT P^T ([B] x [F], K = r d), dP = x^T dT ([F] x [r d],
K = B), dE = S^T h ([|E|] x [d], K = B).  A K-sliced T or dx with 2 - 8 slices is summed by k_tr_fc_post_slices<NS> or
k_tr_bn1_bwd_sums<NS>, more slices by k_tg_reduce.

The oracle costs 1.5 - 3.5 s of CPU per step at these shapes (tests/test_train_oracle.py::test_factored_form_is_the_dense_form)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from coper_amd import data as cdata
from tests.test_gpu_train import _train_step_case

pytestmark = pytest.mark.gpu

# fb15k237_cpg's layer dimensions (r = 32, d = 200, F = 4608) on a smaller graph
_FB_DIMS = dict(num_ent=3000, num_rel=40, ent_emb_size=200, rel_emb_size=32, emb_h=10, emb_w=20, conv_num_channels=32,
                context_rel_conv=None, context_rel_out=[])


def _full(name):
    md = dict(cdata.CONFIGS[name])
    md.pop("queries", None)
    return md


@pytest.mark.parametrize("B,clip_norm", [
    # T and dx in 18 and 25 K slices summed by k_tg_reduce; dP with KS16 = 3 (one whole round of the three-buffer main loop, no tail)
    pytest.param(48, 5.0, id="B48"),
    # T in 6 slices (k_tr_fc_post_slices<6>), dx in 9 (k_tg_reduce); three row tiles: the fourth wave of each workgroup returns early;
    # dP with a tail of one k-step
    pytest.param(300, 5.0, id="B300"),
    # T in 5 slices (<5>), dx in 7 (k_tr_bn1_bwd_sums<7>); a ragged last row tile (389 = 3 x 128 + 5); dP tail of one k-step.
    # The global norm (0.4, then 0.12) is above clip_norm: the clip scale takes the sum of squares the w128 epilogue accumulates for dP
    pytest.param(389, 0.05, id="B389_clipped"),
    # T in 2 slices (<2>), dx in 3 (k_tr_bn1_bwd_sums<3>); dE cut into K slices on the four-wave kernel, so it stays off the side stream
    pytest.param(1000, 5.0, id="B1000"),
])
def test_fb15k237_dims_step_matches_oracle(B, clip_norm):
    norms = _train_step_case("fb15k237_dims", True, False, "n0.1", B=B, L=37, steps=2, case=_FB_DIMS, form="factored",
                             clip_norm=clip_norm)
    if clip_norm < 5.0:
        assert min(norms) > 2 * clip_norm, norms


# the device's step-0 gradients of the full-size cases, for test_w128_route_is_taken
_DEFAULT_GRADS = {}

_FULL = {
    # the step bench.py times: T in 5 slices (<5>), dx in 7 (bn1_bwd_sums<7>), dP with a two-k-step tail; dE and dP on the side
    # streams; the fused scorer k_tr_score_loss_dh at L = 1000
    "fb15k237_cpg": dict(one_vs_all=False),
    # T in 18 slices (k_tg_reduce), dx in 6 (bn1_bwd_sums<6>); dE on the w128 kernel on the side stream with a ragged last row
    # tile (40,943 rows) and a two-k-step tail; k_tr_build_S in two LDS stretches
    "wn18rr_cpg": dict(one_vs_all=False),
    # 1-vs-all: S = h E^T, dE = S^T h and dh = S E all on the w128 kernel, dh in 128 K slices (k_tg_reduce).
    # (Batches 100 / 101 are not used here: at step 1 one kept conv activation of query 29 lies 6.4e-8 from its ReLU's kink, inside
    # the fp32 rounding of the conv and Conv1BN, so the device took either side of it from run to run -- a discontinuity of the
    # function, not a fault of a kernel: 1 % of the ent_emb gradient's largest entry in row e1[29], 7e-4 of conv1_weights'.  With
    # 300 / 301 the kept conv activations stay >= 3.2e-7 from the kink at both steps, as in the other full-size cases.)
    "wn18rr_cpg-one_vs_all": dict(one_vs_all=True, batch_seed=300),
}


def _full_size_step(tag, grads_out=None):
    name = tag.split("-")[0]
    _train_step_case(name, True, _FULL[tag]["one_vs_all"], "n0.1", B=512, L=1000, steps=2, case=_full(name), form="factored",
                     grads_out=grads_out, batch_seed=_FULL[tag].get("batch_seed", 100))


@pytest.mark.parametrize("tag", sorted(_FULL))
def test_full_size_step_matches_oracle(tag):
    g = {}
    _full_size_step(tag, g)
    _DEFAULT_GRADS[tag] = g


_ROUTE_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from tests.test_gpu_train_large import _full_size_step
g = {}
_full_size_step(%(tag)r, g)
np.savez(%(out)r, **{k.replace("/", "|"): v for k, v in g.items()})
"""

# gradients that one of the step's GEMMs on the w128 kernel computes, or that are computed from one
_W128_LEAVES = {
    "fb15k237_cpg": ["fc_weights/CPG/Projection0", "rel_emb", "conv1_weights"],      # dP; T (the contexts); dx
    "wn18rr_cpg": ["fc_weights/CPG/Projection0", "rel_emb", "conv1_weights", "ent_emb"],   # ... and dE
}


@pytest.mark.parametrize("tag", sorted(_W128_LEAVES))
def test_w128_route_is_taken(tag, tmp_path):
    """The kernel choice depends on the shape alone, so a case could pass without reaching the kernel it is there for.  A fresh
    process with COPER_TG_NO_W128=1 (read once per process) runs the same full-size step on the four-wave kernel: it meets the
    oracle's bounds too, and its gradients differ in some bits from the default process's -- bit-identical ones would mean that the
    w128 kernel never ran.  COPER_DBG_POISON=0xFF fills every allocation of the child's library with NaN patterns, so that a
    slice or tile nobody wrote cannot pass on stale memory."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "grads.npz")
    env = dict(os.environ, COPER_TG_NO_W128="1", COPER_DBG_POISON="0xFF")
    child = subprocess.run([sys.executable, "-c", _ROUTE_CHILD % dict(root=root, tag=tag, out=out)], env=env, capture_output=True,
                           text=True, timeout=600)
    assert child.returncode == 0, child.stderr[-4000:]
    assert "COPER_TG_NO_W128" not in os.environ
    four = {k.replace("|", "/"): v for k, v in np.load(out).items()}
    if tag not in _DEFAULT_GRADS:          # (run on its own: the default route's step again)
        g = {}
        _full_size_step(tag, g)
        _DEFAULT_GRADS[tag] = g
    w128 = _DEFAULT_GRADS[tag]
    assert sorted(four) == sorted(w128)
    for leaf in _W128_LEAVES[tag]:
        assert not np.array_equal(four[leaf], w128[leaf]), leaf
