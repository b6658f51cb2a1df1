"""CPU: coper_config.dense_mode (COPER_DENSE_FACTORED, the generated dense layer without the per-relation weight cache) through the
binding and coper_create's validation.  No compute calls here."""
import ctypes as C

import pytest

from coper_amd import _lib, data as cdata

EUNSUPPORTED, EINVAL = 7, 1
X3 = dict(score_mode=_lib.SCORE_BF16X3)


def _create(md, **kw):
    lib = _lib.load()
    cfg = _lib.make_config(md, **kw)
    h = C.c_void_p()
    rc = lib.coper_create(C.byref(cfg), C.byref(h))
    return lib, rc, h


def _specs(lib, h):
    out = {}
    for i in range(lib.coper_num_params(h)):
        nm, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert lib.coper_param_spec(h, i, C.byref(nm), shape, C.byref(nd)) == 0
        out[nm.value.decode()] = tuple(shape[j] for j in range(nd.value))
    return out


def test_config_round_trip_and_struct_size():
    md = cdata.model_descriptors("fb15k237_cpg")
    assert (_lib.DENSE_CACHED, _lib.DENSE_FACTORED) == (0, 1)
    assert _lib.make_config(md).dense_mode == _lib.DENSE_CACHED
    cfg = _lib.make_config(md, dense_mode=_lib.DENSE_FACTORED, role=_lib.ROLE_ENCODE, rel_mod=(1, 0), **X3)
    assert (cfg.dense_mode, cfg.role, cfg.rel_mod_world, cfg.rel_mod_rank) == (_lib.DENSE_FACTORED, _lib.ROLE_ENCODE, 1, 0)
    # the field took the last reserved slot: the struct is the 192 bytes it was with `int32_t reserved[1]` at its end
    assert C.sizeof(_lib.coper_config) == 192
    assert _lib.coper_config.dense_mode.offset == C.sizeof(_lib.coper_config) - 4
    assert _lib.coper_config.rel_mod_rank.offset == C.sizeof(_lib.coper_config) - 8
    assert _lib.COPER_ABI_VERSION == 3


@pytest.mark.parametrize("name,over,kw", [
    ("fb15k237_cpg", {}, {}),
    ("wn18rr_cpg", {}, {}),
    ("nations_cpg", {}, {}),
    ("synth10m_cpg", {}, {}),
    ("fb15k237_cpg", dict(context_rel_out=[64]), {}),                       # g_MLP
    ("fb15k237_cpg", dict(context_rel_out=[64], context_rel_use_batch_norm=True), {}),
    ("fb15k237_cpg", dict(context_rel_conv=[]), {}),                        # generated conv filters
    ("fb15k237_cpg", dict(context_rel_conv=[16], context_rel_out=[64]), {}),
    ("fb15k237_cpg", dict(concat_rel=True), {}),
    ("nations_cpg", {}, dict(role=_lib.ROLE_ENCODE)),
    ("nations_cpg", {}, dict(rel_mod=(1, 0))),
])
def test_factored_is_accepted(name, over, kw):
    md = cdata.model_descriptors(name, **over)
    lib, rc, h = _create(md, dense_mode=_lib.DENSE_FACTORED, **X3, **kw)
    assert rc == 0, lib.coper_last_error(None)
    fac = _specs(lib, h)
    lib.coper_destroy(h)
    lib, rc, h = _create(md, **X3, **kw)
    assert rc == 0
    assert _specs(lib, h) == fac == {k: tuple(v) for k, v in cdata.param_shapes(md).items()}     # same leaves, same shapes
    lib.coper_destroy(h)


@pytest.mark.parametrize("name,over,kw,frag", [
    ("fb15k237_plain", {}, X3, "not generated"),
    ("fb15k237_cpg", dict(do_parameter_lookup=True, context_rel_conv=[]), X3, "g_lookup"),
    ("fb15k237_cpg", dict(context_rel_out=None, context_rel_conv=[]), X3, "not generated"),      # generated conv, static dense
    ("fb15k237_cpg", {}, dict(score_mode=_lib.SCORE_F32), "COPER_SCORE_BF16X3"),
    ("fb15k237_cpg", {}, dict(role=_lib.ROLE_SCORE, **X3), "COPER_ROLE_SCORE"),
    ("fb15k237_cpg", {}, dict(rel_mod=(2, 0), **X3), "rel_mod_world"),
])
def test_factored_is_refused_with_a_reason(name, over, kw, frag):
    md = cdata.model_descriptors(name, **over)
    lib, rc, h = _create(md, **kw)
    assert rc == 0, lib.coper_last_error(None)          # the configuration itself is fine: cached mode takes it
    lib.coper_destroy(h)
    lib, rc, h = _create(md, dense_mode=_lib.DENSE_FACTORED, **kw)
    assert rc == EUNSUPPORTED and not h.value
    msg = lib.coper_last_error(None).decode()
    assert msg and "COPER_DENSE_FACTORED" in msg and frag in msg


@pytest.mark.parametrize("mode", [7, -1, 2])
def test_unknown_dense_mode_is_invalid(mode):
    lib, rc, h = _create(cdata.model_descriptors("fb15k237_cpg"), dense_mode=mode, **X3)
    assert rc == EINVAL and not h.value
    assert "dense_mode" in lib.coper_last_error(None).decode()


def test_factored_handle_state_errors_need_no_device():
    lib, rc, h = _create(cdata.model_descriptors("nations_cpg"), dense_mode=_lib.DENSE_FACTORED, **X3)
    assert rc == 0
    assert lib.coper_encode(h, None, None, 4, None, None, None) == 5          # ESTATE: not prepared
    assert lib.coper_prepare(h, None) == 2                                    # EMISSING
    lib.coper_destroy(h)
