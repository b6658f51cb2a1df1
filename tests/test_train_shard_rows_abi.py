"""Deferred rows on an entity shard (include/coper_hip.h, "Deferred rows" and "Entity-sharded training") arrive with ONE
new symbol, coper_train_rows_updates; every touched call keeps its argument types, the ABI version and coper_train_config are what
they were.  No GPU: a handle is created (coper_create touches no device) and never initialised for training, so what is reachable
here are the refusals that need no device."""
import ctypes
import os
import re

from coper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = 1, 5
_P, _I64, _I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32

# the symbols the mode touches on a sharded state, as include/coper_hip.h declares them
TOUCHED = {
    "coper_train_defer_rows": (ctypes.c_int, [_P, _I32, _P]),
    "coper_train_rows_deferred": (ctypes.c_int, [_P]),
    "coper_train_rows_updates": (_I64, [_P]),
    "coper_train_sync_rows": (ctypes.c_int, [_P, _P]),
    "coper_train_row_stats": (ctypes.c_int, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64), _P]),
    "coper_train_shard_gather": (ctypes.c_int, [_P, _P, _I64, _P, _P]),
    "coper_train_shard_forward": (ctypes.c_int, [_P, _P, _P, _P, _I64, _P, _P]),
    "coper_train_shard_score_csr": (ctypes.c_int, [_P, _P, _P, _P, _I64, _I64, _P, _P, _P]),
    "coper_train_shard_score_lookup": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _P, _P]),
    "coper_train_shard_backward": (ctypes.c_int, [_P, _P, _P, _I32, _P, _P, _P]),
    "coper_train_shard_apply": (ctypes.c_int, [_P, _P, _I32, _P]),
}


def _header():
    return open(os.path.join(ROOT, "include", "coper_hip.h")).read()


def _shard_handle(lib):
    from coper_amd import data as cdata
    md = dict(cdata._COMMON)
    md.update(num_ent=37, num_rel=3, ent_emb_size=40, rel_emb_size=8, emb_h=10, emb_w=4, conv_num_channels=4, context_rel_conv=None,
              context_rel_out=[])
    cfg = _lib.make_config(md, shard=(8, 29))
    h = ctypes.c_void_p()
    assert lib.coper_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    return h


def test_the_touched_calls_keep_their_argument_types():
    text = _header()
    for name, proto in TOUCHED.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert len(re.findall(r"COPER_API\s+\w+\s+%s\s*\(" % name, text)) == 1, name
    assert re.search(r"COPER_API\s+int\s+coper_train_defer_rows\s*\(\s*coper_handle\s*\*\s*h\s*,\s*int32_t\s+enable\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert re.search(r"COPER_API\s+int64_t\s+coper_train_rows_updates\s*\(\s*const\s+coper_handle\s*\*\s*h\s*\)", text)
    assert re.search(r"COPER_API\s+int\s+coper_train_shard_gather\s*\(\s*coper_handle\s*\*\s*h\s*,\s*const\s+int64_t\s*\*\s*e1\s*,\s*int64_t\s+B\s*,"
                     r"\s*float\s*\*\s*rows_out\s*,\s*void\s*\*\s*stream\s*\)", text)


def test_the_header_no_longer_lists_the_mode_as_not_built():
    text = _header()
    sharded = text[text.index("Entity-sharded training"):]
    not_built = sharded[sharded.index("Not built:"):]
    not_built = not_built[:not_built.index("*/")]
    assert "deferred rows on a shard" not in not_built
    assert "row-block split step" in not_built      # what the mode leaves open is named there instead
    assert "Deferred rows on a shard" in sharded[:sharded.index("Not built:")]


def test_the_new_symbol_is_exported():
    lib = _lib.load()      # (load() binds every prototype: a missing export raises here)
    assert lib.coper_train_rows_updates is not None


def test_null_handles():
    lib = _lib.load()
    assert lib.coper_train_defer_rows(None, 1, None) == EINVAL
    assert lib.coper_train_rows_deferred(None) == -EINVAL
    assert lib.coper_train_rows_updates(None) == -EINVAL
    assert lib.coper_train_sync_rows(None, None) == EINVAL
    assert lib.coper_train_row_stats(None, None, None, None, None) == EINVAL
    assert lib.coper_train_shard_gather(None, None, 1, None, None) == EINVAL
    assert lib.coper_train_shard_score_csr(None, None, None, None, 1, 1, None, None, None) == EINVAL
    assert lib.coper_train_shard_backward(None, None, None, 1, None, None, None) == EINVAL
    assert lib.coper_train_shard_apply(None, None, 1, None) == EINVAL


def test_before_train_init_every_call_is_estate():
    lib = _lib.load()
    h = _shard_handle(lib)
    try:
        assert lib.coper_train_defer_rows(h, 1, None) == ESTATE and b"coper_train_init" in lib.coper_last_error(h)
        assert lib.coper_train_rows_deferred(h) == -ESTATE
        assert lib.coper_train_rows_updates(h) == -ESTATE
        assert lib.coper_train_sync_rows(h, None) == ESTATE
        assert lib.coper_train_row_stats(h, None, None, None, None) == ESTATE
        for rc in (lib.coper_train_shard_gather(h, None, 1, None, None), lib.coper_train_shard_forward(h, None, None, None, 1, None, None),
                   lib.coper_train_shard_score_csr(h, None, None, None, 1, 1, None, None, None),
                   lib.coper_train_shard_score_lookup(h, None, None, 1, 1, None, None, None),
                   lib.coper_train_shard_backward(h, None, None, 1, None, None, None), lib.coper_train_shard_apply(h, None, 1, None)):
            assert rc == ESTATE and b"coper_train_init_sharded" in lib.coper_last_error(h)
    finally:
        lib.coper_destroy(h)


def test_abi_version_is_unchanged():
    assert _lib.load().coper_abi_version() == 3 == _lib.COPER_ABI_VERSION
    assert ctypes.sizeof(_lib.coper_train_config) == 80
    assert int(re.search(r"#define\s+COPER_ABI_VERSION\s+(\d+)", _header()).group(1)) == 3
