"""CPU: the wide training entry points of the 192-wide deformation block (geom_deform_layer_wide_fwd_f32,
geom_deform_layer_wide_bwd_f32: 17 .. 64 meshes as ceil(b / 16) row tiles per vertex) refuse bad argument structs on the host,
before anything is enqueued: -1 = GEOM_EINVAL, -3 = GEOM_EUNSUPPORTED, 0 = the empty-shape return.

In the manner of test_deform_train_host.py: every row is one valid struct at b = 17 with the named fields changed; no row is a
valid call (the pointers lie in a host buffer that is never dereferenced, and a struct that passed every check would be
launched).  b <= 16 belongs to the plain entry points and is GEOM_EUNSUPPORTED here; every other check answers as theirs do."""
import ctypes

import pytest

from geometrics_amd import _lib, deform

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
    """A forward layer with a product (s_in p0 -> s_out p13) at 17 meshes, training mode, no residual, no tail, no head."""
    a = _lib.DeformFwd(17, 482, 192, 64, 8, *map(_value, ("p0", "p1", "p2", "p3")), None, None,
                       *map(_value, ("p4", "p5", "p6", "p7")), 1, 0.1, 1e-5, 1, None, 0, 0.5,
                       *map(_value, ("p8", "p9", "p10", "p11", "p12", "p13")), None, None, 0)
    return _apply(a, edits)


def _bwd(**edits):
    """A backward layer below another (dz_up p0, product into ds_up p3) at 17 meshes, no residual, no tail, no head."""
    a = _lib.DeformBwd(17, 482, 192, 64, 8, *map(_value, ("p0", "p1", "p2")), None, None, *map(_value, ("p3", "p4")),
                       None, None, 0, 0, *map(_value, ("p5", "p6", "p7", "p8", "p9")), 1, 0, 0.5,
                       None, *map(_value, ("p10", "p11", "p12", "p13")), None, None, None, None, 0)
    return _apply(a, edits)


_TOP = dict(dz_up=None, ell_col_t=None, ell_val_t=None, ds_up=None, wt_up=None, g="p14")     # the top layer: gradient from memory

FWD_ROWS = [
    (dict(b=16), -3),
    (dict(b=1), -3),
    (dict(b=65), -3),
    (dict(b=-1), -1),
    (dict(b=0), 0),
    (dict(nv=0), 0),
    (dict(b=0, s_in=None), 0),
    (dict(nv=0, x_out="p9+4"), 0),
    (dict(c=0), -1),                      # (the shape check answers first)
    (dict(c=191), -3),
    (dict(k=32), -3),
    (dict(ell_w=16), -3),
    (dict(nv=1 << 26), -3),
    (dict(s_in=None), -1),
    (dict(ell_col=None), -1),
    (dict(ell_val=None), -1),
    (dict(x_out=None), -1),
    (dict(save_mean=None), -1),
    (dict(save_invstd=None), -1),
    (dict(s_out=None), -1),
    (dict(w_head="p15", s_head="p16"), -1),
    (dict(tail_col="p17"), -1),
    (dict(res="p18", res_ld=191), -1),
    (dict(res="p18", res_ld=70000), -3),            # 17 * 482 * 70000 >= 2^29: the residual's 32-bit byte offsets
    (dict(res="p18", res_ld=70000, s_in=None), -1),  # (the operand checks answer first)
    (dict(s_in="p0+4"), -1),
    (dict(ell_col="p2+4"), -1),
    (dict(x_out="p9+4"), -1),
    (dict(z_out="p8+4"), -1),
    (dict(s_out="p13+4"), -1),
    (dict(bias="p1+4"), -1),
    (dict(res="p18+2", res_ld=192), -1),
    (dict(w_next="p12+4"), -1),
    (dict(b=16, x_out=None), -3),
    (dict(b=65, s_in=None), -3),
    (dict(c=0, b=65), -1),
]

BWD_ROWS = [
    (dict(b=16), -3),
    (dict(b=65), -3),
    (dict(b=-1), -1),
    (dict(b=0), 0),
    (dict(nv=0), 0),
    (dict(b=0, z=None), 0),
    (dict(c=0), -1),
    (dict(c=191), -3),
    (dict(k=32), -3),
    (dict(ell_w=16), -3),
    (dict(nv=1 << 26), -3),
    (dict(z=None), -1),
    (dict(save_mean=None), -1),
    (dict(save_invstd=None), -1),
    (dict(dz=None), -1),
    (dict(ell_col_t=None), -1),
    (dict(ell_val_t=None), -1),
    (dict(ds_up=None), -1),
    (dict(wt_up=None), -1),
    (dict(ds_head="p15", w_head="p16"), -1),
    (dict(tail_col_t="p17"), -1),
    (dict(g2="p18", g2_ld=191), -1),
    (dict(g2="p18", g2_ld=70000), -3),
    (dict(dz_up="p0+4"), -1),
    (dict(ds_up="p3+4"), -1),
    (dict(g2="p18+2", g2_ld=192), -1),
    (dict(z="p5+4"), -1),
    (dict(grad_res="p19+4", has_res=1), -1),
    (dict(dz="p10+4"), -1),
    (dict(colsum="p13+4"), -1),
    (dict(wt_up="p4+4"), -1),
    (dict(b=16, dz="p10+4"), -3),
]

BWD_TOP_ROWS = [
    (dict(b=16), -3),
    (dict(b=65), -3),
    (dict(b=0), 0),
    (dict(g=None), -1),
    (dict(g=None, ds_head="p15"), -1),
    (dict(g=None, ds_head="p15", w_head="p16", dw_head="p17"), -1),
    (dict(ds_head="p15", w_head="p16", x_top="p18+4"), -1),
    (dict(g="p14+2", g_ld=192), -1),
    (dict(g_ld=191), -1),
    (dict(z=None), -1),
]


def _is_refusal(edits, code):
    """Nothing here may reach a launch: a refusal, or the empty-shape return of an empty shape."""
    return code in (-1, -3) or (code == 0 and (edits.get("b") == 0 or edits.get("nv") == 0))


_ids = lambda v: ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None      # noqa: E731


@pytest.mark.parametrize("edits,code", FWD_ROWS, ids=_ids)
def test_wide_forward_refusals(edits, code):
    assert _is_refusal(edits, code)
    assert _lib.lib().geom_deform_layer_wide_fwd_f32(ctypes.byref(_fwd(**edits)), None) == code


@pytest.mark.parametrize("edits,code", BWD_ROWS, ids=_ids)
def test_wide_backward_refusals(edits, code):
    assert _is_refusal(edits, code)
    assert _lib.lib().geom_deform_layer_wide_bwd_f32(ctypes.byref(_bwd(**edits)), None) == code


@pytest.mark.parametrize("edits,code", BWD_TOP_ROWS, ids=_ids)
def test_wide_top_layer_backward_refusals(edits, code):
    assert _is_refusal(edits, code)
    assert _lib.lib().geom_deform_layer_wide_bwd_f32(ctypes.byref(_bwd(**dict(_TOP, **edits))), None) == code


def test_null_structs_and_the_interface_version():
    L = _lib.lib()
    assert L.geom_deform_layer_wide_fwd_f32(None, None) == -1 and L.geom_deform_layer_wide_bwd_f32(None, None) == -1
    # the two families split the batch sizes: each refuses the other's valid struct
    assert L.geom_deform_layer_fwd_f32(ctypes.byref(_fwd()), None) == -3 and L.geom_deform_layer_wide_fwd_f32(ctypes.byref(_fwd(b=16)), None) == -3
    assert L.geom_deform_layer_bwd_f32(ctypes.byref(_bwd()), None) == -3 and L.geom_deform_layer_wide_bwd_f32(ctypes.byref(_bwd(b=16)), None) == -3
    assert L.geom_abi_version() == 16 and _lib.ABI_VERSION == 16
    assert deform.WIDE_MAX_BATCH == 64
