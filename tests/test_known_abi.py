"""The known-facts entry points without a GPU: coper_set_known_facts, coper_known_filter, coper_predict_topk_known and
coper_encode_rank_known are declared, exported and bound, and the argument validation that needs no device returns the documented
codes (include/coper_hip.h)."""
import ctypes as C
import inspect
import os
import re

import pytest

from coper_amd import _lib
from coper_amd import data as cdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE, EUNSUPPORTED = 1, 5, 7
SYMBOLS = (("coper_set_known_facts", 8), ("coper_known_filter", 9), ("coper_predict_topk_known", 9), ("coper_encode_rank_known", 10))


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
    for name, nargs in SYMBOLS:
        m = re.search(r"COPER_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs, name
    # sizes are int64, k int32, *nnz a pointer to int64, everything else a plain pointer
    a = _lib.PROTOTYPES["coper_set_known_facts"][1]
    assert a[5] is C.c_int64 and a[6] is C.c_int64
    a = _lib.PROTOTYPES["coper_known_filter"][1]
    assert a[3] is C.c_int64 and a[6] is C.c_int64 and a[7] is C.POINTER(C.c_int64)
    a = _lib.PROTOTYPES["coper_predict_topk_known"][1]
    assert a[4] is C.c_int64 and a[5] is C.c_int32
    assert _lib.PROTOTYPES["coper_encode_rank_known"][1][5] is C.c_int64
    assert "#define COPER_ABI_VERSION 3" in header          # symbols were added, no struct changed


def test_argument_validation_needs_no_device(lib):
    one = C.c_void_p(4096)      # a non-null address that is never dereferenced: every call below is refused before any device work
    nnz = C.c_int64(7)
    # a NULL handle
    assert lib.coper_set_known_facts(None, one, one, one, one, 1, 1, None) == EINVAL
    assert lib.coper_known_filter(None, one, one, 1, one, None, 0, C.byref(nnz), None) == EINVAL
    assert lib.coper_predict_topk_known(None, one, one, None, 1, 1, one, one, None) == EINVAL
    assert lib.coper_encode_rank_known(None, one, one, None, one, 1, None, one, None, None) == EINVAL
    h = _handle(lib)
    try:
        # negative sizes
        assert lib.coper_set_known_facts(h, one, one, one, one, -1, 1, None) == EINVAL
        assert lib.coper_set_known_facts(h, one, one, one, one, 1, -1, None) == EINVAL
        assert b"coper_set_known_facts" in lib.coper_last_error(h)
        assert lib.coper_known_filter(h, one, one, -1, one, None, 0, C.byref(nnz), None) == EINVAL
        assert lib.coper_known_filter(h, one, one, 1, one, one, -1, C.byref(nnz), None) == EINVAL
        assert lib.coper_predict_topk_known(h, one, one, None, -1, 1, one, one, None) == EINVAL
        assert lib.coper_encode_rank_known(h, one, one, None, one, -1, None, one, None, None) == EINVAL
        # k <= 0
        assert lib.coper_predict_topk_known(h, one, one, None, 1, 0, one, one, None) == EINVAL
        assert lib.coper_predict_topk_known(h, one, one, None, 1, -2, one, one, None) == EINVAL
        # e1 forms the key: e1_rows alone does not do
        assert lib.coper_predict_topk_known(h, None, one, one, 1, 1, one, one, None) == EINVAL
        assert lib.coper_encode_rank_known(h, None, one, one, one, 1, None, one, None, None) == EINVAL
        assert b"e1" in lib.coper_last_error(h)
        # well-formed, but the handle was never prepared
        assert lib.coper_predict_topk_known(h, one, one, None, 1, 1, one, one, None) == ESTATE
        assert lib.coper_encode_rank_known(h, one, one, None, one, 1, None, one, None, None) == ESTATE
        assert b"coper_prepare" in lib.coper_last_error(h)
        # no index set
        assert lib.coper_known_filter(h, one, one, 1, one, None, 0, C.byref(nnz), None) == ESTATE
        assert b"coper_set_known_facts" in lib.coper_last_error(h)
        # removing an index that was never set touches no device
        assert lib.coper_set_known_facts(h, None, None, None, None, 0, 0, None) == 0
    finally:
        lib.coper_destroy(h)
    h = _handle(lib, role=_lib.ROLE_ENCODE)
    try:
        assert lib.coper_set_known_facts(h, one, one, one, one, 1, 1, None) == EUNSUPPORTED
        assert b"COPER_ROLE_ENCODE" in lib.coper_last_error(h)
    finally:
        lib.coper_destroy(h)


def test_python_wrappers_exist_with_the_documented_signature():
    from coper_amd.fact_network import FactNetworkScorer
    from coper_amd.kg_loader import TSVKGLoader
    from coper_amd.models import ConvE
    assert list(inspect.signature(ConvE.set_known_facts).parameters) == ["self", "e1", "rel", "tail_indptr", "tail_idx"]
    assert list(inspect.signature(ConvE.known_filter).parameters) == ["self", "e1", "rel"]
    sig = inspect.signature(ConvE.predict_topk_known)
    assert list(sig.parameters) == ["self", "e1", "rel", "k", "e1_rows"] and sig.parameters["e1_rows"].default is None
    sig = inspect.signature(ConvE.rank_pass_known)
    assert list(sig.parameters) == ["self", "e1", "rel", "e2", "want_equal", "e1_rows"]
    assert sig.parameters["want_equal"].default is True and sig.parameters["e1_rows"].default is None
    sig = inspect.signature(TSVKGLoader.known_facts)
    assert sig.parameters["splits"].default == ("train", "dev", "test") and sig.parameters["include_inv_relations"].default is True
    assert callable(cdata.known_facts_from_queries) and callable(FactNetworkScorer.set_known_facts)
