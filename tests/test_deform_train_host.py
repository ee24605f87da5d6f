"""CPU: the four training entry points of the 192-wide deformation block (geom_deform_layer_fwd_f32, geom_deform_layer_bwd_f32,
geom_deform_chain_fwd_f32, geom_deform_chain_bwd_f32) refuse bad argument structs on the host, before anything is enqueued, and
with the code they have always answered: -1 = GEOM_EINVAL, -3 = GEOM_EUNSUPPORTED, 0 = the empty-shape return.

Every row is one valid struct with the named fields changed.  The expected codes were recorded from the library as it stood
before the checks were gathered into db_check_fwd / db_check_bwd (csrc/deform_block.hip) and are literals: for a struct with
several faults the FIRST failing check decides, so the rows with two faults pin the order of the checks.  No row is a valid
call: the pointers lie in a host buffer that is never dereferenced, and a struct that passed every check would be launched.

A pointer value is written "pN" (slot N of the buffer, 128-byte aligned) or "pN+B" (B bytes further: misaligned)."""
import ctypes

import pytest

from geometrics_amd import _lib

_BUF = ctypes.create_string_buffer(64 * 128 + 128)
_BASE = (ctypes.addressof(_BUF) + 127) & ~127


def _value(v):
    if not isinstance(v, str):
        return v
    slot, _, off = v[1:].partition("+")
    return _BASE + 128 * int(slot) + int(off or 0)


def _apply(a, edits):
    for field, v in edits.items():
        setattr(a, field, _value(v))
    return a


def _fwd(**edits):
    """A forward layer with a product (s_in p0 -> s_out p13), training mode, no residual, no tail, no head."""
    a = _lib.DeformFwd(16, 482, 192, 64, 8, *map(_value, ("p0", "p1", "p2", "p3")), None, None,
                       *map(_value, ("p4", "p5", "p6", "p7")), 1, 0.1, 1e-5, 1, None, 0, 0.5,
                       *map(_value, ("p8", "p9", "p10", "p11", "p12", "p13")), None, None, 0)
    return _apply(a, edits)


def _bwd(**edits):
    """A backward layer below another (dz_up p0, product into ds_up p3), no residual, no tail, no head."""
    a = _lib.DeformBwd(16, 482, 192, 64, 8, *map(_value, ("p0", "p1", "p2")), None, None, *map(_value, ("p3", "p4")),
                       None, None, 0, 0, *map(_value, ("p5", "p6", "p7", "p8", "p9")), 1, 0, 0.5,
                       None, *map(_value, ("p10", "p11", "p12", "p13")), None, None, None, None, 0)
    return _apply(a, edits)


_TOP = dict(dz_up=None, ell_col_t=None, ell_val_t=None, ds_up=None, wt_up=None, g="p14")     # the top layer: gradient from memory

# (edits, code of geom_deform_layer_fwd_f32, code of geom_deform_chain_fwd_f32 with the edits on the middle of three layers)
FWD_ROWS = [
    (dict(b=17), -3, -3),
    (dict(b=-1), -1, -1),
    (dict(b=0), 0, -1),
    (dict(nv=0), 0, -1),
    (dict(nv=-1), -1, -1),
    (dict(c=191), -3, -3),
    (dict(c=384), -3, -3),
    (dict(c=0), -1, -1),
    (dict(k=32), -3, -3),
    (dict(k=-1), -1, -1),
    (dict(ell_w=16), -3, -3),
    (dict(nv=1 << 26), -3, -3),
    (dict(s_in=None), -1, -1),
    (dict(ell_col=None), -1, -1),
    (dict(ell_val=None), -1, -1),
    (dict(x_out=None), -1, -1),
    (dict(save_mean=None), -1, -1),
    (dict(save_invstd=None), -1, -1),
    (dict(training=0, run_mean=None), -1, -1),
    (dict(training=0, run_var=None), -1, -1),
    (dict(s_out=None), -1, -1),
    (dict(w_head="p15"), -1, -1),
    (dict(s_head="p16"), -1, -1),
    (dict(w_head="p15", s_head="p16"), -1, -1),
    (dict(tail_col="p17"), -1, -1),
    (dict(res="p18", res_ld=191), -1, -1),
    (dict(res="p18", res_ld=0), -1, -1),
    (dict(res="p18", res_ld=70000), -3, -3),              # 16 * 482 * 70000 >= 2^29: the residual's 32-bit byte offsets
    (dict(res="p18", res_ld=70000, s_in=None), -1, -1),   # (the operand checks answer first)
    (dict(s_in="p0+4"), -1, -1),
    (dict(ell_col="p2+4"), -1, -1),
    (dict(ell_val="p3+4"), -1, -1),
    (dict(x_out="p9+4"), -1, -1),
    (dict(z_out="p8+4"), -1, -1),
    (dict(s_out="p13+4"), -1, -1),
    (dict(bias="p1+4"), -1, -1),
    (dict(res="p18+2", res_ld=192), -1, -1),
    (dict(w_next="p12+4"), -1, -1),
    (dict(c=191, s_in=None), -3, -3),
    (dict(b=17, x_out=None), -3, -3),
    (dict(nv=1 << 26, ell_col=None), -3, -3),
    (dict(c=0, b=17), -1, -1),
    (dict(b=0, s_in=None), 0, -1),
    (dict(nv=0, x_out="p9+4"), 0, -1),
]

# (edits on top of _bwd(), code of geom_deform_layer_bwd_f32, code of geom_deform_chain_bwd_f32 with the edits on layers[1])
BWD_ROWS = [
    (dict(b=17), -3, -3),
    (dict(b=-1), -1, -1),
    (dict(b=0), 0, -1),
    (dict(nv=0), 0, -1),
    (dict(nv=-1), -1, -1),
    (dict(c=191), -3, -3),
    (dict(c=384), -3, -3),
    (dict(c=0), -1, -1),
    (dict(k=32), -3, -3),
    (dict(k=-1), -1, -1),
    (dict(ell_w=16), -3, -3),
    (dict(nv=1 << 26), -3, -3),
    (dict(z=None), -1, -1),
    (dict(save_mean=None), -1, -1),
    (dict(save_invstd=None), -1, -1),
    (dict(dz=None), -1, -1),
    (dict(ell_col_t=None), -1, -1),
    (dict(ell_val_t=None), -1, -1),
    (dict(ds_up=None), -1, -1),
    (dict(wt_up=None), -1, -1),
    (dict(ds_head="p15", w_head="p16"), -1, -1),
    (dict(tail_col_t="p17"), -1, -1),
    (dict(g2="p18", g2_ld=191), -1, -1),
    (dict(g2="p18", g2_ld=70000), -3, -3),
    (dict(g_ld=191), -1, -1),
    (dict(g_ld=70000), -3, -3),
    (dict(dz_up="p0+4"), -1, -1),
    (dict(ell_col_t="p1+4"), -1, -1),
    (dict(ell_val_t="p2+4"), -1, -1),
    (dict(ds_up="p3+4"), -1, -1),
    (dict(g2="p18+2", g2_ld=192), -1, -1),
    (dict(z="p5+4"), -1, -1),
    (dict(grad_res="p19+4", has_res=1), -1, -1),
    (dict(dz="p10+4"), -1, -1),
    (dict(colsum="p13+4"), -1, -1),
    (dict(wt_up="p4+4"), -1, -1),
    (dict(g2="p18", g2_ld=70000, z="p5+4"), -3, -3),
    (dict(g2="p18", g2_ld=70000, z=None), -1, -1),
    (dict(g2="p18", g2_ld=70000, g_ld=191), -1, -1),
    (dict(g2="p18", g2_ld=70000, tail_col_t="p17"), -1, -1),
    (dict(c=191, z=None), -3, -3),
    (dict(b=17, dz="p10+4"), -3, -3),
    (dict(b=0, z=None), 0, -1),
]

# ... the same for the top layer (_bwd(**_TOP)), in the chain on layers[0]
BWD_TOP_ROWS = [
    (dict(b=17), -3, -3),
    (dict(b=0), 0, -1),
    (dict(c=191), -3, -3),
    (dict(g=None), -1, -1),
    (dict(g=None, ds_head="p15"), -1, -1),
    (dict(g=None, ds_head="p15", w_head="p16", dw_head="p17"), -1, -1),
    (dict(ds_head="p15", w_head="p16", x_top="p18+4"), -1, -1),
    (dict(g="p14+2", g_ld=192), -1, -1),
    (dict(g_ld=191), -1, -1),
    (dict(g_ld=70000), -3, -3),
    (dict(g_ld=70000, g="p14+2"), -3, -3),
    (dict(g_ld=70000, save_mean=None), -1, -1),
    (dict(z=None), -1, -1),
    (dict(dz="p10+4"), -1, -1),
    (dict(colsum="p13+4"), -1, -1),
]


def _is_refusal(edits, code):
    """Nothing here may reach a launch: a refusal, or the empty-shape return of an empty shape."""
    return code in (-1, -3) or (code == 0 and (edits.get("b") == 0 or edits.get("nv") == 0))


def _fwd_chain(edits=None, at=1, last_product=False):
    """Three linked forward layers p0 -> p13 -> p20, the last without a product (last_product: with one, written where the
    layer before it wrote: no ping-pong)."""
    s = [_fwd(), _fwd(s_in="p13", s_out="p20"), _fwd(s_in="p20", w_next=None, s_out=None)]
    if last_product:
        _apply(s[2], dict(w_next="p12", s_out="p20"))
    if edits:
        _apply(s[at], edits)
    return (_lib.DeformFwd * 3)(*s)


def _bwd_chain(edits=None, at=1):
    """Three linked backward layers: the top one (dz p10), then dz_up p10 -> dz p21, dz_up p21 -> dz p22."""
    s = [_bwd(**_TOP), _bwd(dz_up="p10", dz="p21"), _bwd(dz_up="p21", dz="p22")]
    if edits:
        _apply(s[at], edits)
    return (_lib.DeformBwd * 3)(*s)


def _chain_fwd_code(structs, count=3, done="p30"):
    return _lib.lib().geom_deform_chain_fwd_f32(count, ctypes.addressof(structs) if structs is not None else None, _value(done), None)


def _chain_bwd_code(structs, count=3, done="p31", ds_first="p32"):
    return _lib.lib().geom_deform_chain_bwd_f32(count, ctypes.addressof(structs) if structs is not None else None, _value(done),
                                                _value(ds_first), None)


@pytest.mark.parametrize("edits,layer,chain", FWD_ROWS, ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_forward_refusals(edits, layer, chain):
    assert _is_refusal(edits, layer) and chain in (-1, -3)
    assert _lib.lib().geom_deform_layer_fwd_f32(ctypes.byref(_fwd(**edits)), None) == layer
    assert _chain_fwd_code(_fwd_chain(edits)) == chain


@pytest.mark.parametrize("edits,layer,chain", BWD_ROWS, ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_backward_refusals(edits, layer, chain):
    assert _is_refusal(edits, layer) and chain in (-1, -3)
    assert _lib.lib().geom_deform_layer_bwd_f32(ctypes.byref(_bwd(**edits)), None) == layer
    assert _chain_bwd_code(_bwd_chain(edits)) == chain


@pytest.mark.parametrize("edits,layer,chain", BWD_TOP_ROWS, ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_top_layer_backward_refusals(edits, layer, chain):
    assert _is_refusal(edits, layer) and chain in (-1, -3)
    assert _lib.lib().geom_deform_layer_bwd_f32(ctypes.byref(_bwd(**dict(_TOP, **edits))), None) == layer
    assert _chain_bwd_code(_bwd_chain(edits, at=0)) == chain


def test_null_structs():
    L = _lib.lib()
    assert L.geom_deform_layer_fwd_f32(None, None) == -1 and L.geom_deform_layer_bwd_f32(None, None) == -1
    assert _chain_fwd_code(None) == -1 and _chain_bwd_code(None) == -1


# what only a chain can get wrong: (keyword arguments of the call, edits, layer they go on, code)
FWD_CHAIN_ROWS = [
    (dict(count=0), {}, 0, -1),
    (dict(count=14), {}, 0, -1),
    (dict(done=None), {}, 0, -1),
    (dict(done="p30+64"), {}, 0, -1),
    ({}, dict(s_in="p23"), 1, -1),
    ({}, dict(s_in="p23"), 2, -1),
    (dict(last_product=True), {}, 0, -1),
    ({}, dict(w_next=None, s_out=None), 0, -1),
    ({}, dict(w_next=None, s_out=None), 1, -1),
    ({}, dict(ell_col="p24"), 1, -1),
    ({}, dict(ell_val="p24"), 2, -1),
    ({}, dict(tail_col="p24", tail_val="p25"), 1, -1),
    ({}, dict(nv=480), 2, -1),
    ({}, dict(b=8), 1, -1),
    ({}, dict(b=0), 0, -1),
    ({}, dict(b=17), 2, -3),
    (dict(count=1), dict(b=17), 0, -3),
    (dict(count=1), dict(x_out=None), 0, -1),
    (dict(count=2), dict(z_out="p8+4"), 1, -1),
    (dict(done="p30+64"), dict(c=191), 0, -1),
    ({}, dict(s_in="p23", c=191), 1, -3),
    ({}, dict(s_in="p23", x_out=None), 1, -1),
    ({}, dict(res="p18", res_ld=70000), 1, -3),
    ({}, dict(res="p18", res_ld=70000), 2, -3),
    ({}, dict(res="p18", res_ld=70000, x_out=None), 1, -1),
    ({}, dict(s_in="p23", res="p18", res_ld=70000), 1, -1),   # (the chain's links are checked in front of a layer's operands)
]
BWD_CHAIN_ROWS = [
    (dict(count=0), {}, 0, -1),
    (dict(count=14), {}, 0, -1),
    (dict(done=None), {}, 0, -1),
    (dict(done="p31+64"), {}, 0, -1),
    (dict(count=1), {}, 0, -1),
    (dict(ds_first="p32+4"), {}, 0, -1),
    ({}, dict(dz_up="p0"), 0, -1),
    ({}, dict(dz_up=None, g="p14"), 1, -1),
    ({}, dict(dz_up="p23"), 1, -1),
    ({}, dict(dz_up="p23"), 2, -1),
    ({}, dict(dz="p10"), 2, -1),
    ({}, dict(dz="p21"), 2, -1),
    ({}, dict(ell_col_t="p24"), 2, -1),
    ({}, dict(ell_val_t="p24"), 2, -1),
    ({}, dict(tail_col_t="p24", tail_val_t="p25"), 2, -1),
    ({}, dict(nv=480), 2, -1),
    ({}, dict(b=8), 1, -1),
    ({}, dict(b=0), 0, -1),
    (dict(count=1, ds_first=None), dict(z=None), 0, -1),
    (dict(count=1, ds_first=None), dict(c=191), 0, -3),
    ({}, dict(dz="p10", g2="p18", g2_ld=70000), 2, -3),
    ({}, dict(dz_up="p23", g2="p18", g2_ld=70000), 2, -1),
    ({}, dict(ell_col_t="p24", g2="p18", g2_ld=70000), 2, -1),
    (dict(ds_first="p32+4"), dict(c=191), 0, -1),
]


def _empty(structs, field="b"):
    for s in structs:
        setattr(s, field, 0)
    return structs


@pytest.mark.parametrize("call,edits,at,code", FWD_CHAIN_ROWS)
def test_forward_chain_refusals(call, edits, at, code):
    assert code in (-1, -3)
    call = dict(call)
    structs = _fwd_chain(edits, at, last_product=call.pop("last_product", False))
    assert _chain_fwd_code(structs, **call) == code


@pytest.mark.parametrize("call,edits,at,code", BWD_CHAIN_ROWS)
def test_backward_chain_refusals(call, edits, at, code):
    assert code in (-1, -3)
    assert _chain_bwd_code(_bwd_chain(edits, at), **call) == code


def test_empty_chains_return_after_the_whole_loop():
    """b == 0 / nv == 0 on every layer: 0, but only once every layer has passed its checks (the layer entry points return
    before they look at a pointer)."""
    for field in ("b", "nv"):
        assert _chain_fwd_code(_empty(_fwd_chain(), field)) == 0
        assert _chain_bwd_code(_empty(_bwd_chain(), field)) == 0
        assert _chain_fwd_code(_empty(_fwd_chain(dict(x_out=None)), field)) == -1
        assert _chain_bwd_code(_empty(_bwd_chain(dict(z=None)), field)) == -1
        assert _chain_bwd_code(_empty(_bwd_chain(dict(g2="p15", g2_ld=70000, z="p5+4")), field)) == -1
