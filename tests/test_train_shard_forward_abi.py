"""Forward-only calls on an entity-sharded training state (include/coper_hip.h, "Entity-sharded training": "Forward-only calls";
DESIGN 6.12) arrive with TWO new symbols, coper_train_shard_forward_lookup and coper_train_shard_forward_csr; the ABI version and
coper_train_config are what they were.  No GPU: a handle is created (coper_create touches no device) and never initialised for
training, so what is reachable here are the refusals that need no device."""
import ctypes
import os
import re

from coper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = 1, 5
_P, _I64 = ctypes.c_void_p, ctypes.c_int64

# (h, e1, rel, e1_rows, lookup, labels, B, L, loss_part, pred_part, h_out, stream)
# (h, e1, rel, e1_rows, lab_indptr, lab_idx, lab_row, n_rows, B, loss_part, pred_local, h_out, stream)
NEW = {
    "coper_train_shard_forward_lookup": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I64, _P, _P, _P, _P]),
    "coper_train_shard_forward_csr": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _P, _P, _P, _P]),
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


def test_the_new_symbols_are_declared_once_with_these_argument_types():
    text = _header()
    for name, proto in NEW.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert len(re.findall(r"COPER_API\s+\w+\s+%s\s*\(" % name, text)) == 1, name
    ptr = lambda c, t, n: r"\s*%s%s\s*\*\s*%s\s*" % ("const\\s+" if c else "", t, n)
    head = r"\s*coper_handle\s*\*\s*h\s*," + ptr(1, "int64_t", "e1") + "," + ptr(1, "int64_t", "rel") + "," + ptr(1, "float", "e1_rows") + ","
    assert re.search(r"COPER_API\s+int\s+coper_train_shard_forward_lookup\s*\(" + head + ptr(1, "int32_t", "lookup") + "," + ptr(1, "float", "labels") +
                     r",\s*int64_t\s+B\s*,\s*int64_t\s+L\s*," + ptr(0, "double", "loss_part") + "," + ptr(0, "float", "pred_part") + "," +
                     ptr(0, "float", "h_out") + "," + ptr(0, "void", "stream") + r"\)", text)
    assert re.search(r"COPER_API\s+int\s+coper_train_shard_forward_csr\s*\(" + head + ptr(1, "int64_t", "lab_indptr") + "," + ptr(1, "int64_t", "lab_idx") +
                     "," + ptr(1, "int64_t", "lab_row") + r",\s*int64_t\s+n_rows\s*,\s*int64_t\s+B\s*," + ptr(0, "double", "loss_part") + "," +
                     ptr(0, "float", "pred_local") + "," + ptr(0, "float", "h_out") + "," + ptr(0, "void", "stream") + r"\)", text)


def test_the_new_symbols_are_exported():
    lib = _lib.load()      # (load() binds every prototype: a missing export raises here)
    for name in NEW:
        assert getattr(lib, name) is not None


def test_the_header_no_longer_lists_a_forward_only_call_as_not_built():
    text = _header()
    sharded = text[text.index("Entity-sharded training"):]
    assert sharded.count("Not built:") == 1
    before, not_built = sharded[:sharded.index("Not built:")], sharded[sharded.index("Not built:"):]
    not_built = not_built[:not_built.index("*/")]
    assert "forward-only" not in not_built
    assert "row-block split step" in not_built      # what stays open is still named there
    assert "Deferred rows on a shard" in before
    # the contract of the two calls stands above the sentence
    for word in ("coper_train_shard_forward_lookup(", "coper_train_shard_forward_csr(", "loss_part", "pred_part", "pred_local", "nothing is written"):
        assert word in before, word


def test_null_handles():
    lib = _lib.load()
    assert lib.coper_train_shard_forward_lookup(None, None, None, None, None, None, 1, 1, None, None, None, None) == EINVAL
    assert lib.coper_train_shard_forward_csr(None, None, None, None, None, None, None, 1, 1, None, None, None, None) == EINVAL


def test_before_train_init_sharded_both_calls_are_estate():
    lib = _lib.load()
    h = _shard_handle(lib)
    try:
        for rc in (lib.coper_train_shard_forward_lookup(h, None, None, None, None, None, 1, 1, None, None, None, None),
                   lib.coper_train_shard_forward_csr(h, None, None, None, None, None, None, 1, 1, None, None, None, None)):
            assert rc == ESTATE and b"coper_train_init_sharded" in lib.coper_last_error(h)
        assert b"coper_train_shard_forward_csr" in lib.coper_last_error(h)      # (the text names the call that was refused)
    finally:
        lib.coper_destroy(h)


def test_abi_version_is_unchanged():
    assert _lib.load().coper_abi_version() == 3 == _lib.COPER_ABI_VERSION
    assert ctypes.sizeof(_lib.coper_train_config) == 80
    assert int(re.search(r"#define\s+COPER_ABI_VERSION\s+(\d+)", _header()).group(1)) == 3
