"""The deferred-rows mode arrives as four new symbols (include/coper_hip.h, "Deferred rows"): coper_train_config gains no field, its
size and COPER_ABI_VERSION are what they were.  No GPU: a handle is created (coper_create touches no device) and never initialised
for training."""
import ctypes
import os
import re

from coper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("coper_train_defer_rows", "coper_train_rows_deferred", "coper_train_sync_rows", "coper_train_row_stats")
EINVAL, ESTATE = 1, 5


def _header():
    return open(os.path.join(ROOT, "include", "coper_hip.h")).read()


def test_symbols_are_declared_and_bound():
    text = _header()
    for name in SYMBOLS:
        assert re.search(r"COPER_API\s+int\s+%s\s*\(" % name, text), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.PROTOTYPES["coper_train_defer_rows"][1] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    assert _lib.PROTOTYPES["coper_train_row_stats"][1][1:4] == [ctypes.POINTER(ctypes.c_int64)] * 3


def test_symbols_are_exported():
    lib = _lib.load()      # (load() binds every prototype: a missing export raises here)
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


def test_struct_and_version_are_unchanged():
    assert ctypes.sizeof(_lib.coper_train_config) == 80
    names = [n for n, _ in _lib.coper_train_config._fields_] + [n for n, _ in _lib._coper_train_config_tail._fields_]
    assert not any("row" in n or "defer" in n for n in names), names
    version = int(re.search(r"#define\s+COPER_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert version == 3 == _lib.COPER_ABI_VERSION


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.coper_train_defer_rows(None, 1, None) == EINVAL
    assert lib.coper_train_sync_rows(None, None) == EINVAL
    assert lib.coper_train_row_stats(None, None, None, None, None) == EINVAL
    assert lib.coper_train_rows_deferred(None) == -EINVAL


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
        assert lib.coper_train_defer_rows(h, 1, None) == ESTATE
        assert b"coper_train_init" in lib.coper_last_error(h)
        assert lib.coper_train_sync_rows(h, None) == ESTATE
        assert lib.coper_train_row_stats(h, None, None, None, None) == ESTATE
        assert lib.coper_train_rows_deferred(h) == -ESTATE
    finally:
        lib.coper_destroy(h)
