"""Synchronised batch statistics arrive as new symbols (include/coper_hip.h, "Synchronised batch statistics: the backward in phases"):
coper_train_config gains no field, its size, its tail names and COPER_ABI_VERSION are what they were.  No GPU: a handle is created
(coper_create touches no device) and never initialised for training."""
import ctypes
import os
import re

from coper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("coper_train_sync_begin", "coper_train_sync_begin_csr", "coper_train_sync_next", "coper_train_sync_phase",
           "coper_train_sync_part_len")
EINVAL, ESTATE = 1, 5
_P, _I64, _I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
_PI64 = ctypes.POINTER(ctypes.c_int64)


def _header():
    return open(os.path.join(ROOT, "include", "coper_hip.h")).read()


def test_symbols_are_declared_and_bound():
    text = _header()
    assert "Synchronised batch statistics: the backward in phases" in text
    for name in SYMBOLS:
        assert re.search(r"COPER_API\s+int(64_t)?\s+%s\s*\(" % name, text), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"coper_train_sync_begin\s*\(\s*coper_handle\s*\*\s*h\s*,\s*const\s+int64_t\s*\*\s*e1\s*,\s*const\s+int64_t\s*\*\s*rel\s*,"
                     r"\s*const\s+int32_t\s*\*\s*lookup\s*,\s*const\s+float\s*\*\s*labels\s*,\s*int64_t\s+B\s*,\s*int64_t\s+L\s*,"
                     r"\s*int64_t\s+B_global\s*,\s*int64_t\s+sample_offset\s*,\s*int32_t\s+rows\s*,\s*double\s*\*\s*part_out\s*,"
                     r"\s*int64_t\s+part_cap\s*,\s*int64_t\s*\*\s*n_out\s*,\s*float\s*\*\s*loss_out\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert re.search(r"coper_train_sync_next\s*\(\s*coper_handle\s*\*\s*h\s*,\s*const\s+double\s*\*\s*parts_in\s*(/\*.*?\*/)?\s*,\s*int32_t\s+G\s*,"
                     r"\s*double\s*\*\s*part_out\s*,\s*int64_t\s+part_cap\s*,\s*int64_t\s*\*\s*n_out\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert re.search(r"COPER_API\s+int64_t\s+coper_train_sync_part_len\s*\(\s*const\s+coper_handle\s*\*\s*h\s*\)", text)
    P = _lib.PROTOTYPES
    assert P["coper_train_sync_begin"] == (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I32, _P, _I64, _PI64, _P, _P])
    assert P["coper_train_sync_begin_csr"] == (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _I64, _PI64, _P, _P])
    assert P["coper_train_sync_next"] == (ctypes.c_int, [_P, _P, _I32, _P, _I64, _PI64, _P])
    assert P["coper_train_sync_phase"] == (ctypes.c_int, [_P])
    assert P["coper_train_sync_part_len"] == (_I64, [_P])


def test_symbols_are_exported():
    lib = _lib.load()      # (load() binds every prototype: a missing export raises here)
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


def test_null_handle_is_einval():
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    assert lib.coper_train_sync_begin(None, None, None, None, None, 1, 1, 1, 0, 0, None, 0, ctypes.byref(n), None, None) == EINVAL
    assert lib.coper_train_sync_begin_csr(None, None, None, None, None, None, 1, 1, 1, 0, None, 0, ctypes.byref(n), None, None) == EINVAL
    assert lib.coper_train_sync_next(None, None, 1, None, 0, ctypes.byref(n), None) == EINVAL
    assert lib.coper_train_sync_phase(None) == -EINVAL
    assert lib.coper_train_sync_part_len(None) == -EINVAL
    assert n.value == -1      # (nothing was written)


def test_before_train_init():
    from coper_amd import data as cdata
    lib = _lib.load()
    md = dict(cdata._COMMON)
    md.update(num_ent=37, num_rel=3, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=4, context_rel_conv=None,
              context_rel_out=[])
    cfg = _lib.make_config(md)
    h = ctypes.c_void_p()
    assert lib.coper_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        n = ctypes.c_int64(-1)
        assert lib.coper_train_sync_phase(h) == -ESTATE
        assert lib.coper_train_sync_part_len(h) == 2 * 40      # (the configuration alone: 2 * max(conv_num_channels, ent_emb_size))
        for call in (lambda: lib.coper_train_sync_begin(h, None, None, None, None, 1, 1, 1, 0, 0, None, 0, ctypes.byref(n), None, None),
                     lambda: lib.coper_train_sync_begin_csr(h, None, None, ctypes.byref(n), None, None, 1, 1, 1, 0, None, 0, ctypes.byref(n), None,
                                                            None),
                     lambda: lib.coper_train_sync_next(h, None, 1, None, 0, ctypes.byref(n), None)):
            assert call() == ESTATE
            assert b"coper_train_init" in lib.coper_last_error(h)
    finally:
        lib.coper_destroy(h)


def test_struct_and_version_are_unchanged():
    assert ctypes.sizeof(_lib.coper_train_config) == 80
    assert [n for n, _ in _lib._coper_train_config_tail._fields_] == ["deterministic", "reserved"]
    names = [n for n, _ in _lib.coper_train_config._fields_]
    assert not any("sync" in n for n in names), names
    version = int(re.search(r"#define\s+COPER_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert version == 3 == _lib.COPER_ABI_VERSION
