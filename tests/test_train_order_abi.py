"""Ordered rows arrive as two new symbols (include/coper_hip.h, "Ordered rows"): coper_train_config gains no field, its size, its tail
names and COPER_ABI_VERSION are what they were.  No GPU: a handle is created (coper_create touches no device) and never initialised
for training."""
import ctypes
import os
import re

from coper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("coper_train_order_rows", "coper_train_rows_ordered")
EINVAL, ESTATE = 1, 5


def _header():
    return open(os.path.join(ROOT, "include", "coper_hip.h")).read()


def kernel_constants():
    """The constants of the ordered-rows kernels that the edge cases of tests/test_gpu_train_ordered.py sit on, read from the header."""
    text = _header()
    return {name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) for name in ("COPER_ORDER_SORT_TILE", "COPER_ORDER_SUMSQ_ROWS")}


def test_symbols_are_declared_and_bound():
    text = _header()
    assert re.search(r"COPER_API\s+int\s+coper_train_order_rows\s*\(\s*coper_handle\s*\*\s*h\s*,\s*int32_t\s+enable\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert re.search(r"COPER_API\s+int\s+coper_train_rows_ordered\s*\(\s*const\s+coper_handle\s*\*\s*h\s*\)", text)
    assert _lib.PROTOTYPES["coper_train_order_rows"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p])
    assert _lib.PROTOTYPES["coper_train_rows_ordered"] == (ctypes.c_int, [ctypes.c_void_p])
    assert "Ordered rows" in text


def test_symbols_are_exported():
    lib = _lib.load()      # (load() binds every prototype: a missing export raises here)
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.coper_train_order_rows(None, 1, None) == EINVAL
    assert lib.coper_train_rows_ordered(None) == -EINVAL


def test_before_train_init_is_estate():
    from coper_amd import data as cdata
    lib = _lib.load()
    md = dict(cdata._COMMON)
    md.update(num_ent=37, num_rel=3, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=4, context_rel_conv=None,
              context_rel_out=[])
    cfg = _lib.make_config(md)
    h = ctypes.c_void_p()
    assert lib.coper_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        assert lib.coper_train_order_rows(h, 1, None) == ESTATE
        assert b"coper_train_init" in lib.coper_last_error(h)
        assert lib.coper_train_rows_ordered(h) == -ESTATE
    finally:
        lib.coper_destroy(h)


def test_struct_and_version_are_unchanged():
    assert ctypes.sizeof(_lib.coper_train_config) == 80
    assert [n for n, _ in _lib._coper_train_config_tail._fields_] == ["deterministic", "reserved"]
    names = [n for n, _ in _lib.coper_train_config._fields_]
    assert not any("order" in n for n in names), names
    version = int(re.search(r"#define\s+COPER_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert version == 3 == _lib.COPER_ABI_VERSION


def test_kernel_constants_are_in_the_header():
    k = kernel_constants()
    assert k["COPER_ORDER_SORT_TILE"] % 256 == 0 and k["COPER_ORDER_SORT_TILE"] >= 256
    assert k["COPER_ORDER_SUMSQ_ROWS"] % 4 == 0 and k["COPER_ORDER_SUMSQ_ROWS"] >= 4
