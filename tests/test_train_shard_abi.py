"""Entity-sharded training arrives as new symbols (include/coper_hip.h, "Entity-sharded training"): coper_train_config gains no
field, its size, its tail names and COPER_ABI_VERSION are what they were.  No GPU: a handle is created (coper_create touches no
device) and never initialised for training."""
import ctypes
import os
import re

from coper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("coper_train_init_sharded", "coper_train_sharded", "coper_train_shard_gather", "coper_train_shard_forward",
           "coper_train_shard_score_csr", "coper_train_shard_backward", "coper_train_shard_apply")
EINVAL, ESTATE = 1, 5
_P, _I64 = ctypes.c_void_p, ctypes.c_int64


def _header():
    return open(os.path.join(ROOT, "include", "coper_hip.h")).read()


def test_symbols_are_declared_and_bound():
    text = _header()
    assert "Entity-sharded training" in text
    for name in SYMBOLS:
        assert re.search(r"COPER_API\s+int\s+%s\s*\(" % name, text), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"coper_train_init_sharded\s*\(\s*coper_handle\s*\*\s*h\s*,\s*const\s+coper_train_config\s*\*\s*cfg\s*\)", text)
    assert re.search(r"coper_train_shard_backward\s*\(\s*coper_handle\s*\*\s*h\s*,\s*const\s+float\s*\*\s*dh_parts\s*,\s*const\s+double\s*\*\s*loss_parts\s*,"
                     r"\s*int32_t\s+G\s*,\s*float\s*\*\s*loss_out\s*,\s*double\s*\*\s*sumsq_part\s*,\s*void\s*\*\s*stream\s*\)", text)
    P = _lib.PROTOTYPES
    assert P["coper_train_init_sharded"] == (ctypes.c_int, [_P, ctypes.POINTER(_lib.coper_train_config)])
    assert P["coper_train_sharded"] == (ctypes.c_int, [_P])
    assert P["coper_train_shard_forward"] == (ctypes.c_int, [_P, _P, _P, _P, _I64, _P, _P])
    assert P["coper_train_shard_score_csr"] == (ctypes.c_int, [_P, _P, _P, _P, _I64, _I64, _P, _P, _P])
    assert P["coper_train_shard_backward"] == (ctypes.c_int, [_P, _P, _P, ctypes.c_int32, _P, _P, _P])
    assert P["coper_train_shard_apply"] == (ctypes.c_int, [_P, _P, ctypes.c_int32, _P])


def test_symbols_are_exported():
    lib = _lib.load()      # (load() binds every prototype: a missing export raises here)
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


def test_null_handle_is_einval():
    lib = _lib.load()
    cfg = _lib.coper_train_config()
    assert lib.coper_train_init_sharded(None, ctypes.byref(cfg)) == EINVAL
    assert lib.coper_train_sharded(None) == -EINVAL
    assert lib.coper_train_shard_gather(None, None, 1, None, None) == EINVAL
    assert lib.coper_train_shard_forward(None, None, None, None, 1, None, None) == EINVAL
    assert lib.coper_train_shard_score_csr(None, None, None, None, 1, 1, None, None, None) == EINVAL
    assert lib.coper_train_shard_backward(None, None, None, 1, None, None, None) == EINVAL
    assert lib.coper_train_shard_apply(None, None, 1, None) == EINVAL


def test_before_train_init_is_estate():
    from coper_amd import data as cdata
    lib = _lib.load()
    md = dict(cdata._COMMON)
    md.update(num_ent=37, num_rel=3, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=4, context_rel_conv=None,
              context_rel_out=[])
    cfg = _lib.make_config(md, shard=(8, 29))
    h = ctypes.c_void_p()
    assert lib.coper_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        assert lib.coper_train_sharded(h) == -ESTATE
        for call in (lambda: lib.coper_train_shard_gather(h, None, 1, None, None),
                     lambda: lib.coper_train_shard_forward(h, None, None, None, 1, None, None),
                     lambda: lib.coper_train_shard_score_csr(h, None, None, None, 1, 1, None, None, None),
                     lambda: lib.coper_train_shard_backward(h, None, None, 1, None, None, None),
                     lambda: lib.coper_train_shard_apply(h, None, 1, None)):
            assert call() == ESTATE
            assert b"coper_train_init_sharded" in lib.coper_last_error(h)
    finally:
        lib.coper_destroy(h)


def test_struct_and_version_are_unchanged():
    assert ctypes.sizeof(_lib.coper_train_config) == 80
    assert [n for n, _ in _lib._coper_train_config_tail._fields_] == ["deterministic", "reserved"]
    names = [n for n, _ in _lib.coper_train_config._fields_]
    assert not any("shard" in n for n in names), names
    version = int(re.search(r"#define\s+COPER_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert version == 3 == _lib.COPER_ABI_VERSION
