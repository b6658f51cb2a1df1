"""coper_predict_topk / coper_predict_stats without a GPU: the symbols are exported and bound, and the argument validation that
needs no device returns the documented codes (include/coper_hip.h)."""
import ctypes as C
import inspect
import os
import re

import pytest

from coper_amd import _lib
from coper_amd import data as cdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE, EUNSUPPORTED = 1, 5, 7


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from coper_amd.build import build_library
        build_library()
    return _lib.load()


def _handle(lib, **kw):
    md = cdata.model_descriptors("nations_cpg")
    cfg = _lib.make_config(md, **kw)
    h = C.c_void_p()
    assert lib.coper_create(C.byref(cfg), C.byref(h)) == 0
    return h


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "coper_hip.h")).read()
    for name, nargs in (("coper_predict_topk", 13), ("coper_predict_stats", 7)):
        m = re.search(r"COPER_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs
        assert hasattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs
    # k is int32, B and filt_nnz int64, everything else a pointer
    args = _lib.PROTOTYPES["coper_predict_topk"][1]
    assert args[7] is C.c_int64 and args[8] is C.c_int64 and args[9] is C.c_int32
    assert all(a is C.c_void_p for i, a in enumerate(args) if i not in (7, 8, 9))


def test_argument_validation_needs_no_device(lib):
    P = C.c_void_p
    one = P(4096)       # a non-null address that is never dereferenced: every call below is refused before any device work
    assert lib.coper_predict_topk(None, one, one, None, None, None, None, 0, 1, 1, one, one, None) == EINVAL
    assert lib.coper_predict_stats(None, 0, None, None, None, None, None) == EINVAL
    h = _handle(lib)
    try:
        call = lambda *a: lib.coper_predict_topk(h, *a)
        assert call(one, one, None, None, None, None, 0, 1, 0, one, one, None) == EINVAL        # k == 0
        assert call(one, one, None, None, None, None, 0, 1, -3, one, one, None) == EINVAL       # k < 0
        assert call(one, one, None, None, None, None, 0, -1, 1, one, one, None) == EINVAL       # B < 0
        assert call(one, one, None, one, None, None, 0, 1, 1, one, one, None) == EINVAL         # both (e1, rel) and hvec
        assert call(None, None, None, None, None, None, 0, 1, 1, one, one, None) == EINVAL      # neither
        assert call(one, None, None, None, None, None, 0, 1, 1, one, one, None) == EINVAL       # e1 without rel
        assert call(None, None, None, one, None, one, 3, 1, 1, one, one, None) == EINVAL        # idx without indptr
        assert call(None, None, None, one, one, None, 3, 1, 1, one, one, None) == EINVAL        # nnz without idx
        assert call(None, None, None, one, None, None, 3, 1, 1, one, one, None) == EINVAL       # nnz without a CSR
        assert b"coper_predict_topk" in lib.coper_last_error(h)
        # well-formed, but the handle was never prepared
        assert call(one, one, None, None, None, None, 0, 1, 1, one, one, None) == ESTATE
        assert call(None, None, None, one, one, one, 3, 1, 10, one, one, None) == ESTATE
        assert call(None, None, None, one, None, None, 0, 0, 10, None, None, None) == ESTATE    # (B == 0 is served by prepared handles only)
        # statistics of a handle that never predicted: zeros, no device touched
        nq, nu, nr, ratio = C.c_int64(7), C.c_int64(7), C.c_int64(7), C.c_float(7.0)
        assert lib.coper_predict_stats(h, 1, C.byref(nq), C.byref(nu), C.byref(nr), C.byref(ratio), None) == 0
        assert (nq.value, nu.value, nr.value, ratio.value) == (0, 0, 0, 0.0)
    finally:
        lib.coper_destroy(h)


def test_python_wrappers_exist_with_the_documented_signature():
    from coper_amd.fact_network import FactNetworkScorer
    from coper_amd.models import ConvE
    from coper_amd import sharding
    sig = inspect.signature(ConvE.predict_topk)
    assert list(sig.parameters) == ["self", "e1", "rel", "k", "filt_indptr", "filt_idx", "e1_rows", "h"]
    assert all(sig.parameters[n].default is None for n in ("filt_indptr", "filt_idx", "e1_rows", "h"))
    assert callable(ConvE.predict_stats)
    assert list(inspect.signature(FactNetworkScorer.predict_topk).parameters)[:4] == ["self", "e1", "r", "k"]
    assert callable(sharding.EntityShardedRanker.predict_topk)
