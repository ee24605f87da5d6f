"""CPU: GEOM_FLAG_NN_SAMPLES_ONLY is refused on the host, before anything is enqueued, where it cannot be honoured -- a surface
scan without a tri scan (the two-sided records go through idx_p) and the truncation mode (its legacy kernels scan both
directions) -- and a NULL sq_gt / idx_p stays GEOM_EINVAL without the flag.  No row is a valid call: the pointers lie in a host
buffer that is never dereferenced (the fused branch is refused for its NULL workspace at the latest).  The same calls on real
buffers, where the flag alone decides between 0 and -1: tests/test_nn_one_direction_gpu.py."""
import ctypes

import pytest

from geometrics_amd import _header, _lib

_BUF = ctypes.create_string_buffer(32 * 128 + 128)
_BASE = (ctypes.addressof(_BUF) + 127) & ~127
_P = lambda slot: _BASE + 128 * slot
ONE, TRUNC, FMA = _lib.FLAG_NN_SAMPLES_ONLY, _lib.FLAG_REF_TAIL_TRUNC, _lib.FLAG_NN_FMA

SCAN = dict(b=8, n_gt=3000, gt=_P(0), num=3000, points=_P(1), sq_gt=_P(2), idx_p=_P(3), sq_pred=_P(4), idx_g=_P(5), nv=2562,
            verts=_P(6), nf=5120, faces=_P(7), tri_order=_P(8), tri_dist=_P(9), option=_P(10), index=_P(11), sq=_P(12),
            closest=_P(13), weights=_P(14), u=_P(15), v=_P(16), coef_sample=1.0, coef_other=1.0, order_scratch=_P(17), flags=0,
            workspace=None, workspace_bytes=0)


def _scan_code(**edits):
    assert set(edits) <= set(SCAN)
    wrote = ctypes.c_int(7)
    code = _lib.lib().geom_surface_scan_f32(*dict(SCAN, **edits).values(), ctypes.byref(wrote), None, None, None)
    assert wrote.value == 0
    return code


def test_the_flag_is_a_new_bit_of_the_header():
    assert ONE == 32 == _header.CONSTANTS["FLAG_NN_SAMPLES_ONLY"]
    others = [v for k, v in _header.CONSTANTS.items() if k.startswith("FLAG_") and k != "FLAG_NN_SAMPLES_ONLY"]
    assert all(v & ONE == 0 for v in others)


@pytest.mark.parametrize("edits", [
    dict(flags=ONE, verts=None),                                # no tri scan: the two-sided records need both directions
    dict(flags=ONE, verts=None, sq_gt=None, idx_p=None),
    dict(flags=ONE | TRUNC),                                    # the truncation mode keeps its own kernels
    dict(flags=ONE | TRUNC, workspace=_P(20), workspace_bytes=2854784),
    dict(flags=ONE | TRUNC | FMA),
    dict(flags=0, sq_gt=None),                                  # without the flag the gt points' outputs are required
    dict(flags=0, idx_p=None),
    dict(flags=FMA, sq_gt=None, idx_p=None),
    dict(flags=ONE, sq_pred=None),                              # the kept direction's outputs are required under the flag too
    dict(flags=ONE, idx_g=None),
], ids=lambda e: ",".join("%s=%s" % (k, "NULL" if v is None else v if k == "flags" else "set") for k, v in e.items()))
def test_surface_scan_refusals(edits):
    assert _scan_code(**edits) == -1


def test_chamfer_nn_refusals():
    nn = lambda r1, i1, r2, i2, flags: _lib.lib().geom_chamfer_nn_f32(1, 4, _P(0), 4, _P(1), r1, i1, r2, i2, flags, None)
    assert nn(_P(2), _P(3), _P(4), _P(5), ONE | TRUNC) == -1
    assert nn(None, None, _P(4), _P(5), ONE | TRUNC) == -1
    assert nn(None, _P(3), _P(4), _P(5), 0) == -1 and nn(_P(2), None, _P(4), _P(5), 0) == -1
    assert nn(None, None, None, _P(5), ONE) == -1 and nn(None, None, _P(4), None, ONE) == -1
    assert _lib.lib().geom_chamfer_nn_f32(0, 4, _P(0), 4, _P(1), None, None, None, None, ONE, None) == 0          # empty batch
    # the culled stand-alone scan is two-directional by contract: any flag but the FMA arithmetic is outside it
    assert _lib.lib().geom_chamfer_nn_culled_f32(1, 4, _P(0), 4, _P(1), None, None, _P(2), _P(3), _P(4), _P(5), ONE, _P(6), None) == \
        _lib.EUNSUPPORTED
