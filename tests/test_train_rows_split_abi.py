"""The split step of the deferred-rows mode arrives as five new symbols (include/coper_hip.h, "Deferred rows: the step in calls"):
coper_train_config gains no field, its size and COPER_ABI_VERSION are what they were.  No GPU: a handle is created (coper_create touches
no device) and never initialised for training.  coper_train_rows_layout needs a training state, as coper_train_grads_layout does, so
what it reports is checked on the GPU (tests/test_gpu_train_rows_split.py)."""
import ctypes
import os
import re

from coper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("coper_train_rows_layout", "coper_train_rows_backward", "coper_train_rows_export", "coper_train_rows_import",
           "coper_train_rows_apply")
EINVAL, ESTATE = 1, 5
P, I64 = ctypes.c_void_p, ctypes.c_int64


def _header():
    return open(os.path.join(ROOT, "include", "coper_hip.h")).read()


def test_symbols_are_declared_and_bound():
    text = _header()
    for name in SYMBOLS:
        decl = re.search(r"COPER_API\s+int\s+%s\s*\(([^;]*)\);" % name, text)
        assert decl, name
        assert name in _lib.PROTOTYPES, name
        assert len(_lib.PROTOTYPES[name][1]) == decl.group(1).count(",") + 1, name      # one ctypes argument per declared one
    assert _lib.PROTOTYPES["coper_train_rows_layout"][1] == [P, ctypes.c_char_p] + [ctypes.POINTER(I64)] * 4
    assert _lib.PROTOTYPES["coper_train_rows_backward"][1] == _lib.PROTOTYPES["coper_train_step"][1]
    assert _lib.PROTOTYPES["coper_train_rows_export"][1] == [P, P, I64, ctypes.c_int32, P, P, I64, P, P]
    assert _lib.PROTOTYPES["coper_train_rows_import"][1] == [P, P, P, I64, ctypes.c_int32, P]
    assert _lib.PROTOTYPES["coper_train_rows_apply"][1] == _lib.PROTOTYPES["coper_train_apply"][1]


def test_symbols_are_exported():
    lib = _lib.load()      # (load() binds every prototype: a missing export raises here)
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


def test_struct_and_version_are_unchanged():
    assert ctypes.sizeof(_lib.coper_train_config) == 80
    version = int(re.search(r"#define\s+COPER_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert version == 3 == _lib.COPER_ABI_VERSION
    assert _lib.load().coper_abi_version() == 3


def test_the_refusals_of_the_dense_split_step_name_the_new_calls():
    """The header's "Deferred rows" block and the library's three refusal messages point at the mode's own split step."""
    text = _header()
    block = text[text.index("/* Deferred rows: an opt-in mode"):text.index("/* Deferred rows: the step in calls")]
    assert "coper_train_rows_backward" in block
    src = open(os.path.join(ROOT, "coper_amd", "csrc", "coper_train.hip")).read()
    assert len(re.findall(r"deferred-rows mode \(coper_train_defer_rows\)[^;]*coper_train_rows_(?:backward|export|apply)", src)) == 3


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.coper_train_rows_layout(None, None, None, None, None, None) == EINVAL
    assert lib.coper_train_rows_backward(None, None, None, None, None, 1, 1, None, None) == EINVAL
    assert lib.coper_train_rows_export(None, None, 0, 0, None, None, 0, None, None) == EINVAL
    assert lib.coper_train_rows_import(None, None, None, 0, 1, None) == EINVAL
    assert lib.coper_train_rows_apply(None, None, 0, 1.0, None) == EINVAL


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
        total, rs = I64(), I64()
        assert lib.coper_train_rows_layout(h, None, None, None, ctypes.byref(total), ctypes.byref(rs)) == ESTATE
        assert b"coper_train_init" in lib.coper_last_error(h)
        assert lib.coper_train_rows_backward(h, None, None, None, None, 1, 1, None, None) == ESTATE
        assert lib.coper_train_rows_export(h, None, 0, 0, None, None, 0, None, None) == ESTATE
        assert lib.coper_train_rows_import(h, None, None, 0, 1, None) == ESTATE
        assert lib.coper_train_rows_apply(h, None, 0, 1.0, None) == ESTATE
        assert b"coper_train_init" in lib.coper_last_error(h)
    finally:
        lib.coper_destroy(h)
