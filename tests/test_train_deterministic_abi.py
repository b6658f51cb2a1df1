"""coper_train_config.deterministic is reserved[0] by name (include/coper_hip.h): the struct's size, the offsets of the fields in front
of it and reserved[6] itself are what they were, so a caller built against the earlier header still passes a valid struct (deterministic = 0).  No GPU."""
import ctypes
import os
import re

from coper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_size_and_offsets_are_unchanged():
    cfg = _lib.coper_train_config
    # thirteen 4-byte fields, one_vs_all_chunk, and the six words of reserved[]: twenty words
    assert ctypes.sizeof(cfg) == 80
    assert cfg.one_vs_all_chunk.offset == 52 and cfg.one_vs_all_chunk.size == 4
    # reserved[6] is where it was, and the new field is its word 0 by name (an anonymous union in the header)
    assert cfg.reserved.offset == 56 and cfg.reserved.size == 6 * 4
    assert cfg.deterministic.offset == 56 and cfg.deterministic.size == 4
    c = cfg()
    assert c.deterministic == 0      # a zero-initialised struct asks for the default mode
    c.deterministic = 1
    assert c.reserved[0] == 1 and list(c.reserved[1:]) == [0] * 5
    c.reserved[0] = 0
    assert c.deterministic == 0


def test_binding_mirrors_the_header():
    text = open(os.path.join(ROOT, "include", "coper_hip.h")).read()
    body = re.search(r"typedef struct coper_train_config \{(.*?)\} coper_train_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    tail = re.search(r"union\s*\{(.*?)\}\s*;", body, re.S)
    assert tail is not None and body[tail.end():].strip() == ""      # the union closes the struct

    def names(decls):
        out = []
        for decl in decls.split(";"):
            decl = decl.strip()
            if decl:
                out += [n.strip().split("[")[0] for n in decl.split(None, 1)[1].split(",")]
        return out
    assert names(body[:tail.start()]) == [name for name, _ in _lib.coper_train_config._fields_[:-1]]
    assert names(tail.group(1)) == [name for name, _ in _lib._coper_train_config_tail._fields_] == ["deterministic", "reserved"]
    assert re.search(r"int32_t\s+reserved\[6\]", tail.group(1))
    assert "coper_train_deterministic" in text and "coper_train_deterministic" in _lib.PROTOTYPES
    version = int(re.search(r"#define\s+COPER_ABI_VERSION\s+(\d+)", text).group(1))
    assert version == _lib.COPER_ABI_VERSION
