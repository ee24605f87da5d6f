"""-m gpu: WHICH ROUTE a surface step takes.  geom_surface_prepare_f32 and geom_surface_scan_f32 decide from the same rule
(csrc/tri_distance.hip: surface_step_fuses) whether the step is one fused launch: a coherent triangle order, no truncation /
brute-force flag, one workgroup per query tile (ws_split == 1) and at least 256 query tiles of 64 gt points.  Were the two to
disagree, the draw launch would write triangle records the scan does not read, or the scan would read records nobody wrote.

Every row calls prepare, then scan, the way ops.draw_samples / ops.SurfaceLoss do (the scan gets GEOM_FLAG_TRI_WS_READY when
prepare wrote the records and the culled Chamfer tiles when prepare wrote the samples' index), and compares the three
out-values -- *prepared, *records_written, tail->finalized -- with what the library answered BEFORE the rule was gathered into
one function.  The tables below are literals worked out from that library's host code (the three values are set on the host);
they have NOT yet been confirmed by running that library on an MI355X.  Whatever the route, the scan's outputs equal
geom_chamfer_nn_f32 + geom_tri_surface_fwd_f32 on the same inputs bit for bit.

Shapes: the 320-face icosphere, 8 meshes, 2048 samples, 1984 / 1985 gt points = 248 / 256 query tiles, the two sides of the
boundary (2048 samples: the sorted draws and the in-launch finalize roles are reachable); the 5120-face icosphere, one mesh,
3000 gt points = 47 tiles, which four workgroups share (the split route).  No row makes a role give up."""
import ctypes
import functools

import pytest
import torch

from geometrics_amd import _lib as L
from geometrics_amd import meshgen, ops
from geometrics_amd.tri_distance import face_order, faces_in_order

pytestmark = pytest.mark.gpu

SHAPES = {"tiles248": (2, 8, 2048, 1984), "tiles256": (2, 8, 2048, 1985), "split4": (4, 1, 2048, 3000)}   # level, b, num, n_gt
FLAGS = {"0": 0, "fix6": L.FLAG_FIX_REGION6, "fma": L.FLAG_NN_FMA, "trunc": L.FLAG_REF_TAIL_TRUNC, "brute": L.FLAG_TRI_BRUTE_FORCE}

# (prepared, records_written, finalized) per flag, in the order of FLAGS, for (order, cull, tail) present (1) or absent (0)
ROUTES = {
    "tiles248": {
        (0, 0, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (0, 0, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (0, 1, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (0, 1, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (1, 0, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (1, 0, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (1, 1, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (1, 1, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
    },
    "tiles256": {
        (0, 0, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (0, 0, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (0, 1, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (0, 1, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (1, 0, 0): [(1, 1, 0), (1, 1, 0), (1, 1, 0), (0, 0, 0), (0, 0, 0)],
        (1, 0, 1): [(1, 1, 0), (1, 1, 0), (1, 1, 0), (0, 0, 0), (0, 0, 0)],
        (1, 1, 0): [(3, 1, 0), (3, 1, 0), (3, 1, 0), (0, 0, 0), (0, 0, 0)],
        (1, 1, 1): [(3, 1, 1), (3, 1, 1), (3, 1, 1), (0, 0, 0), (0, 0, 0)],
    },
    "split4": {
        (0, 0, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (0, 0, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (0, 1, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (0, 1, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (1, 0, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (1, 0, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (1, 1, 0): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
        (1, 1, 1): [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
    },
}


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    level, b, num, n_gt = SHAPES[shape]
    gpu = torch.device("cuda:0")
    V, Fc = meshgen.icosphere(level)
    to = lambda a: torch.from_numpy(a).to(gpu).contiguous()
    verts, faces, gt = to(meshgen.jittered_batch(V, b)), to(Fc), to(meshgen.gt_cloud(b, n_gt))
    return verts, faces, gt, face_order(verts, faces), faces_in_order(verts, faces), ops.GtIndex(gt)


def observe(shape, order, flag, cull, tail):
    """One prepare + scan; returns ((prepared, records_written, finalized), the scan's outputs, the separate entry points')."""
    level, b, num, n_gt = SHAPES[shape]
    verts, faces, gt, tri_order, in_order, gi = _inputs(shape)
    gpu, lib, flags = verts.device, L.lib(), FLAGS[flag]
    nv, nf = verts.shape[1], faces.shape[0]
    f32, i32 = dict(dtype=torch.float32, device=gpu), dict(dtype=torch.int32, device=gpu)
    order_ptr = tri_order.data_ptr() if order else None
    ws_bytes = lib.geom_tri_distance_workspace_bytes(b, n_gt, nf)

    def outputs():
        return dict(sq_gt=torch.empty(b, n_gt, **f32), idx_p=torch.empty(b, n_gt, **i32), sq_pred=torch.empty(b, num, **f32),
                    idx_g=torch.empty(b, num, **i32), tri_dist=torch.empty(b, n_gt, **f32), option=torch.empty(b, n_gt, **i32),
                    index=torch.empty(b, n_gt, **i32), sq=torch.empty(b, n_gt, **f32), closest=torch.empty(b, n_gt, 3, **f32),
                    weights=torch.empty(b, n_gt, 3, **f32), ws=torch.zeros(ws_bytes // 4, **f32))

    a, ref = outputs(), outputs()
    choices = torch.empty(b, num, dtype=torch.int64, device=gpu)
    u, v, points = torch.empty(b, num, **f32), torch.empty(b, num, **f32), torch.empty(b, num, 3, **f32)
    s_index = torch.zeros(max(int(lib.geom_nn_cull_index_floats(b, num)), 4), **f32)
    ops.manual_seed(21)
    prepared = ctypes.c_int(-1)
    draw_cull = L.SurfaceCull(None, None, s_index.data_ptr(), in_order.data_ptr())
    L.check(lib.geom_surface_prepare_f32(b, nv, verts.data_ptr(), nf, faces.data_ptr(), num, ops._rng_state(gpu).data_ptr(),
                                         choices.data_ptr(), u.data_ptr(), v.data_ptr(), points.data_ptr(), n_gt, order_ptr, flags,
                                         a["ws"].data_ptr(), ws_bytes, ctypes.byref(prepared),
                                         ctypes.byref(draw_cull) if cull else None, L.stream_ptr()), "geom_surface_prepare_f32")
    scan_cull = L.SurfaceCull(gi.order.data_ptr(), gi.index.data_ptr(), s_index.data_ptr(), None)
    scratch = torch.zeros(lib.geom_surface_order_words(b, nf, num, n_gt), **i32)
    loss = torch.zeros((), **f32)
    coef_s, coef_o = 3000.0 / (b * num), 3000.0 / (b * n_gt)
    tail_arg = L.SurfaceTail(choices.data_ptr(), coef_s, coef_o, 1, loss.data_ptr(), -1)
    wrote = ctypes.c_int(-1)
    L.check(lib.geom_surface_scan_f32(b, n_gt, gt.data_ptr(), num, points.data_ptr(), a["sq_gt"].data_ptr(), a["idx_p"].data_ptr(),
                                      a["sq_pred"].data_ptr(), a["idx_g"].data_ptr(), nv, verts.data_ptr(), nf, faces.data_ptr(),
                                      order_ptr, a["tri_dist"].data_ptr(), a["option"].data_ptr(), a["index"].data_ptr(),
                                      a["sq"].data_ptr(), a["closest"].data_ptr(), a["weights"].data_ptr(), u.data_ptr(),
                                      v.data_ptr(), coef_s, coef_o, scratch.data_ptr(),
                                      flags | (L.FLAG_TRI_WS_READY if prepared.value & 1 else 0), a["ws"].data_ptr(), ws_bytes,
                                      ctypes.byref(wrote), ctypes.byref(scan_cull) if prepared.value & 2 else None,
                                      ctypes.byref(tail_arg) if tail else None, L.stream_ptr()), "geom_surface_scan_f32")
    nn_flags = flags & (L.FLAG_REF_TAIL_TRUNC | L.FLAG_NN_FMA)
    tri_flags = flags & (L.FLAG_REF_TAIL_TRUNC | L.FLAG_FIX_REGION6 | L.FLAG_TRI_BRUTE_FORCE)
    L.call("geom_chamfer_nn_f32", b, n_gt, gt.data_ptr(), num, points.data_ptr(), ref["sq_gt"].data_ptr(), ref["idx_p"].data_ptr(),
           ref["sq_pred"].data_ptr(), ref["idx_g"].data_ptr(), nn_flags)
    L.call("geom_tri_surface_fwd_f32", b, n_gt, gt.data_ptr(), nv, verts.data_ptr(), nf, faces.data_ptr(), order_ptr,
           ref["tri_dist"].data_ptr(), ref["option"].data_ptr(), ref["index"].data_ptr(), ref["sq"].data_ptr(),
           ref["closest"].data_ptr(), ref["weights"].data_ptr(), tri_flags, ref["ws"].data_ptr(), ws_bytes)
    torch.cuda.synchronize()
    return (prepared.value, wrote.value, tail_arg.finalized if tail else 0), a, ref


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_prepare_and_scan_take_the_recorded_route_and_the_scan_equals_the_separate_scans(gpu, shape):
    assert sorted(ROUTES[shape]) == [(o, c, t) for o in (0, 1) for c in (0, 1) for t in (0, 1)]
    for (order, cull, tail), expected in sorted(ROUTES[shape].items()):
        assert len(expected) == len(FLAGS)
        for flag, route in zip(FLAGS, expected):
            got, a, ref = observe(shape, order, flag, cull, tail)
            print(shape, "order=%d cull=%d tail=%d" % (order, cull, tail), flag, got)
            assert got == route, (order, cull, tail, flag)
            for k in ("sq_gt", "idx_p", "sq_pred", "idx_g", "tri_dist", "option", "index", "sq", "closest", "weights"):
                assert torch.equal(a[k], ref[k]), (order, cull, tail, flag, k)
