"""The sampled score call of the entity-sharded step arrives as one new symbol (include/coper_hip.h, "Entity-sharded training";
DESIGN 6.8): the ABI version and coper_train_config are what they were.  No GPU: a handle is created (coper_create touches no
device) and never initialised for training."""
import ctypes
import os
import re

from coper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "coper_train_shard_score_lookup"
EINVAL, ESTATE = 1, 5
_P, _I64 = ctypes.c_void_p, ctypes.c_int64


def _header():
    return open(os.path.join(ROOT, "include", "coper_hip.h")).read()


def test_the_call_is_declared_with_its_signature_and_bound():
    text = _header()
    assert re.search(r"COPER_API\s+int\s+coper_train_shard_score_lookup\s*\(\s*coper_handle\s*\*\s*h\s*,\s*const\s+int32_t\s*\*\s*lookup\s*,"
                     r"\s*const\s+float\s*\*\s*labels\s*,\s*int64_t\s+B\s*,\s*int64_t\s+L\s*,\s*float\s*\*\s*dh_part\s*,"
                     r"\s*double\s*\*\s*loss_part\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert _lib.PROTOTYPES[NAME] == (ctypes.c_int, [_P, _P, _P, _I64, _I64, _P, _P, _P])
    # the header's contract names it where it belongs: in the step's call order and no longer under "Not built"
    not_built = text[text.index("Not built:", text.index("Entity-sharded training")):]
    assert "sampled labels on a sharded table" not in not_built[:not_built.index("*/")]


def test_the_call_is_exported():
    lib = _lib.load()      # (load() binds every prototype: a missing export raises here)
    assert getattr(lib, NAME) is not None


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.coper_train_shard_score_lookup(None, None, None, 1, 1, None, None, None) == EINVAL


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
        assert lib.coper_train_shard_score_lookup(h, None, None, 1, 1, None, None, None) == ESTATE
        assert b"coper_train_init_sharded" in lib.coper_last_error(h)
    finally:
        lib.coper_destroy(h)


def test_abi_version_is_unchanged():
    assert lib_version() == 3 == _lib.COPER_ABI_VERSION
    assert ctypes.sizeof(_lib.coper_train_config) == 80
    version = int(re.search(r"#define\s+COPER_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert version == 3


def lib_version():
    return _lib.load().coper_abi_version()
