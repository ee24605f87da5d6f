"""-m gpu: the texel -> (vertex, weight) lists the pooling's binning role leaves in the backward workspace (csrc/pooling.hip:
pool_bin_body; layout: include/geom_hip.h), read back and held to the forward pooling's own weights, bit for bit.

The map gradient is a gather over these lists; the tests of that gradient see them only through sums whose fp32 order follows
an atomic cursor.  Here the lists themselves are pinned.  P = the forward pooling of the identity maps of a size (channel t =
the one-hot map of texel t) is the operator the float64 tests of the map gradient use: with a map of ones and zeros the
forward's (A*1)*G, (H*1)*A, (G*1)*B, (B*1)*H are the lists' G*A, A*H, B*G, H*B bit for bit and every other term of the sum is an
exact zero, so there is no tolerance and no vertex is left out.  P itself is held to float64 by
test_pooling_vertex_gradient_gpu.py::test_projection_and_weights_against_float64, and the lists with it."""
import ctypes

import numpy as np
import pytest
import torch

from test_pooling_vertex_gradient_gpu import ragged_inputs, training_inputs
from geometrics_amd import _lib, utils

pytestmark = pytest.mark.gpu

# ragged: 2 x 101 vertices, some clamped on one axis or on both (all-zero weights); a 1 x 1 map (only empty lists), fewer texels
# than the binning workgroup has threads, and 1600 texels (a thread scans seven).  training: 3 x 482 vertices (more than a
# workgroup has threads), the four VGG map sizes, the fullest lists.
CASES = {"ragged": (ragged_inputs, (1, 2, 5, 13, 40)), "training": (training_inputs, (56, 28, 14, 7))}


def binned_workspace(gpu, verts, cam_mat, cam_pos, dims):
    """The backward workspace after geom_pool_features_bwd_ld_f32 on one-channel maps of the sizes `dims` with every map's
    gradient requested (and no vertex gradient), as int32 words on the host."""
    b, nv = verts.shape[:2]
    n = len(dims)
    maps = [torch.zeros(b, 1, d, d, device=gpu) for d in dims]
    gmaps = [torch.empty_like(t) for t in maps]
    grad_out = torch.ones(b, nv, n, device=gpu)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in maps])
    gptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in gmaps])
    chans, cdims = (ctypes.c_int * n)(*[1] * n), (ctypes.c_int * n)(*dims)
    ws_bytes = _lib.lib().geom_pool_features_bwd_workspace_bytes(b, nv, n, cdims)
    assert ws_bytes % 4 == 0
    ws = torch.zeros(ws_bytes // 4, dtype=torch.int32, device=gpu)
    with torch.cuda.device(gpu):
        _lib.call("geom_pool_features_bwd_ld_f32", b, nv, verts.data_ptr(), cam_mat.data_ptr(), cam_pos.data_ptr(), n, ptrs, chans,
                  cdims, grad_out.data_ptr(), 0, gptrs, None, ws.data_ptr(), ws_bytes)
    torch.cuda.synchronize()
    return ws.cpu().numpy()


@pytest.mark.parametrize("case", sorted(CASES))
def test_texel_lists_are_the_forward_weights(gpu, case):
    """Per (mesh, map): the offsets start at 0, never decrease and end at the number of non-zeros of P; texel t's list, as a set
    of (vertex, weight bits), is {(v, bits(P[v, t])) : P[v, t] != 0}; no vertex stands twice in a list."""
    make, dims = CASES[case]
    verts, img_info = make()
    verts = verts.to(gpu)
    cam_mat, cam_pos = utils.batch_camera_info(img_info.to(gpu))
    b, nv = verts.shape[:2]
    ws = binned_workspace(gpu, verts, cam_mat, cam_pos, dims)
    # the layout of include/geom_hip.h
    per_mesh = sum(d * d + 1 for d in dims)
    ent0 = (b * per_mesh * 4 + 15) // 16 * 16 // 4
    ent = b * len(dims) * 4 * nv
    offsets = ws[:b * per_mesh].reshape(b, per_mesh)
    ent_v = ws[ent0:ent0 + ent].reshape(b, len(dims), 4 * nv)
    ent_w = ws[ent0 + ent:ent0 + 2 * ent].reshape(b, len(dims), 4 * nv).view(np.uint32)
    level_off, entries = 0, 0
    for l, d in enumerate(dims):
        texels = d * d
        eye = torch.eye(texels, device=gpu).view(1, texels, d, d).expand(b, -1, -1, -1).contiguous()
        P = utils.batched_pooling([eye], verts, (cam_mat, cam_pos)).cpu().numpy()            # [b, nv, texels]
        for mesh in range(b):
            tag = "%s, mesh %d, map %d x %d" % (case, mesh, d, d)
            offs = offsets[mesh, level_off:level_off + texels + 1].astype(np.int64)
            v_want, t_want = np.nonzero(P[mesh])
            assert offs[0] == 0 and bool((np.diff(offs) >= 0).all()), tag
            assert offs[texels] == v_want.size <= 4 * nv, tag
            total = int(offs[texels])
            t_got = np.searchsorted(offs, np.arange(total), side="right") - 1          # the texel whose list entry e stands in
            v_got = ent_v[mesh, l, :total].astype(np.int64)
            assert bool(((v_got >= 0) & (v_got < nv)).all()), tag
            key_got, key_want = t_got * nv + v_got, t_want.astype(np.int64) * nv + v_want
            assert np.unique(key_got).size == total, tag + ": a vertex stands twice in a list"
            got, want = np.argsort(key_got), np.argsort(key_want)
            assert np.array_equal(key_got[got], key_want[want]), tag + ": (texel, vertex) pairs"
            assert np.array_equal(ent_w[mesh, l, :total][got], P[mesh][v_want, t_want].view(np.uint32)[want]), tag + ": weight bits"
            entries += total
        level_off += texels + 1
    assert entries > 0
