"""-m gpu: utils.ragged_pooling (csrc/pooling.hip's bodies instantiated for per-lane meshes) on a union of
four meshes -- 101, 101, 70 and 0 vertices, their 272 rows interleaved by a seeded permutation, so that the five 64-position
tiles of the grouped list are all exercised and two of them straddle a mesh boundary.

What it is held to: utils.batched_pooling on each mesh alone (EXISTING code: maps blocks[l][m:m+1], camera m) bit for bit for
the features and the position gradient; float64 for the position gradient (helpers.pool_vertex_gradient_close: 8 eps of the
element's term mass + 1 texel-coordinate ulp through every term, vertices within 1e-3 texels of a texel line left out, at most
2 % of a mesh's -- on these inputs 0 or 1 per mesh and map shape, 1 / 70 = 1.4 % at the worst) and for every element of the map
gradient (P^T g with the project's 8 eps * sum |P||g|).  Where a map gradient is compared with another launch's, the order
inside a texel's list follows an atomic cursor in both, so the bar is the 2e-6 of the tensor's largest entry that
test_pooling_with_more_channel_chunks_than_grid_slices uses for re-ordered list sums."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import pool_vertex_gradient_close
from geometrics_amd import _lib, ops, ragged, utils
from test_pooling_vertex_gradient_gpu import RAGGED_SHAPES, TRAINING_SHAPE, WIDE_SHAPE, ragged_inputs, wide_inputs

pytestmark = pytest.mark.gpu

B = 4
SHAPES = {"four_maps": RAGGED_SHAPES["four_maps"], "two_maps": RAGGED_SHAPES["two_maps"], "wide": WIDE_SHAPE, "training": TRAINING_SHAPE}
EPS = float(np.finfo(np.float32).eps)
LIST_ORDER_RTOL = 2e-6


# ---------------------------------------------------------------- the test batch (host tensors, built once and never changed)
class Union:
    """verts [272,3] fp32, vert_mesh [272] int64, img_info [4,3]; vids[m]: the union ids of mesh m's vertices in the mesh's own
    order; local[m]: [V_m,3] its vertices."""


@functools.lru_cache(maxsize=None)
def union():
    two, cams = ragged_inputs()
    third = wide_inputs()[0][1, :70]
    u = Union()
    u.local = [two[0].contiguous(), two[1].contiguous(), third.contiguous(), torch.zeros(0, 3)]
    u.img_info = torch.cat([cams, torch.tensor([[60.0, 30.0, 1.0], [120.0, 10.0, 1.1]])])
    sizes = [int(t.shape[0]) for t in u.local]
    vt = sum(sizes)
    perm = torch.randperm(vt, generator=torch.Generator().manual_seed(4))        # concatenated row -> union row
    u.verts = torch.empty(vt, 3)
    u.verts[perm] = torch.cat(u.local)
    u.vert_mesh = torch.empty(vt, dtype=torch.int64)
    u.vert_mesh[perm] = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    off = np.concatenate(([0], np.cumsum(sizes)))
    u.vids = [perm[off[m]:off[m + 1]] for m in range(B)]
    u.vt, u.sizes = vt, sizes
    # the meshes interleave, and the grouped list's tiles [64, 128) and [192, 256) hold vertices of two meshes each
    assert not bool((u.vert_mesh[1:] >= u.vert_mesh[:-1]).all()) and sizes == [101, 101, 70, 0] and vt == 272
    return u


@functools.lru_cache(maxsize=None)
def maps_and_gradient(shape, seed=32):
    """Seeded N(0, 1) maps [B, c, d, d] and output gradient [Vt, sum c] in union order (host generator)."""
    chans, dims = SHAPES[shape]
    gen = torch.Generator().manual_seed(seed)
    maps = tuple(torch.randn(B, c, d, d, generator=gen) for c, d in zip(chans, dims))
    return maps, torch.randn(union().vt, sum(chans), generator=gen)


def cameras(gpu, img_info=None):
    return utils.batch_camera_info((union().img_info if img_info is None else img_info).to(gpu))


def per_mesh(gpu, maps, verts_local, cams, grad_rows, maps_want_grad=True):
    """utils.batched_pooling on every mesh with vertices ALONE: [(features [V_m, C], verts.grad [V_m,3], map gradients [1,c,d,d]
    or None)]."""
    out = []
    for m, local in enumerate(verts_local):
        if not local.shape[0]:
            out.append(None)
            continue
        v = local.to(gpu)[None].requires_grad_(True)
        mm = [t[m:m + 1].to(gpu).contiguous().requires_grad_(maps_want_grad) for t in maps]
        feats = utils.batched_pooling(mm, v, (cams[0][m:m + 1].contiguous(), cams[1][m:m + 1].contiguous()))
        got = torch.autograd.grad(feats, [v] + (mm if maps_want_grad else []), grad_rows[m].to(gpu)[None])
        out.append((feats.detach()[0], got[0][0], [t for t in got[1:]] if maps_want_grad else None))
    return out


_reference = {}


def reference(gpu, shape):
    """per_mesh for the test batch at `shape`, computed once and shared (device tensors, never changed)."""
    if shape not in _reference:
        u = union()
        maps, g = maps_and_gradient(shape)
        _reference[shape] = per_mesh(gpu, maps, u.local, cameras(gpu), [g[ids] for ids in u.vids])
    return _reference[shape]


def run(gpu, maps, verts, vert_mesh, cams, grad_out, maps_want_grad=True, headroom=0, monkeypatch=None):
    """utils.ragged_pooling forward and backward on the device -> (features, verts.grad, [map gradients] or None).  headroom:
    grad_out handed in as the trailing columns of a buffer that much wider; the pitch the backward launch received is checked."""
    v = verts.to(gpu).requires_grad_(True)
    mm = [t.to(gpu).requires_grad_(maps_want_grad) for t in maps]
    feats = utils.ragged_pooling(mm, v, vert_mesh.to(gpu), cams)
    ctot = grad_out.shape[1]
    wide = torch.zeros(grad_out.shape[0], headroom + ctot, device=gpu)
    wide[:, headroom:] = grad_out.to(gpu)
    pitches, call = [], ops._lib.call

    def recording_call(name, *args):
        if name == "geom_pool_features_ragged_bwd_f32":
            pitches.append(int(args[13]))                    # grad_ld (0 = the pooled width)
        return call(name, *args)

    if monkeypatch is not None:
        monkeypatch.setattr(ops._lib, "call", recording_call)
    got = torch.autograd.grad(feats, [v] + (mm if maps_want_grad else []), wide[:, headroom:])
    if monkeypatch is not None:
        monkeypatch.setattr(ops._lib, "call", call)
        assert pitches == [headroom + ctot if headroom else 0]
    return feats.detach(), got[0], list(got[1:]) if maps_want_grad else None


def same_with_nan(a, b):
    """Equal bit patterns up to which NaN: the NaN masks agree and everything else (the infinities included) is equal."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def close_in_list_order(got, want, what):
    """Two sums of the same terms in another order: NaN and Inf where the other has them, the rest within LIST_ORDER_RTOL of
    the tensor's largest finite entry."""
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want[inf]), what
    fin = torch.isfinite(want)
    if bool(fin.any()):
        scale = float(want[fin].abs().max())
        err = float((got[fin].double() - want[fin].double()).abs().max())
        assert err <= LIST_ORDER_RTOL * max(scale, 1e-30), "%s: max err %g at scale %g" % (what, err, scale)


# ---------------------------------------------------------------- 1, 2: against the per-mesh batched calls, bit for bit
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_features_equal_the_per_mesh_batched_pooling_bit_for_bit(gpu, shape):
    u = union()
    maps, g = maps_and_gradient(shape)
    feats = utils.ragged_pooling([t.to(gpu) for t in maps], u.verts.to(gpu), u.vert_mesh.to(gpu), cameras(gpu))
    assert feats.shape == (u.vt, sum(SHAPES[shape][0])) and feats.is_contiguous()
    for m, ref in enumerate(reference(gpu, shape)):
        if ref is not None:
            assert torch.equal(feats[u.vids[m].to(gpu)], ref[0]), "mesh %d" % m
    # int32 ids and the camera parameters in place of the pair: the same rows
    again = utils.ragged_pooling([t.to(gpu) for t in maps], u.verts.to(gpu), u.vert_mesh.to(gpu, torch.int32), u.img_info.to(gpu))
    assert torch.equal(again, feats)


@pytest.mark.parametrize("maps_want_grad", (True, False), ids=("with_maps", "verts_only"))
@pytest.mark.parametrize("headroom", (0, 7))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_position_gradient_equals_the_per_mesh_one_bit_for_bit(gpu, monkeypatch, shape, headroom, maps_want_grad):
    """A vertex's per-chunk sums are formed by the same waves in the same order whatever tile it sits in, the chunks are added
    in chunk order and their number depends on the channels only.  grad_out contiguous and as the trailing columns of a buffer 7
    columns wider (read pitched, in place), the maps wanting a gradient or not (no binning workgroups, no gather slices)."""
    u = union()
    maps, g = maps_and_gradient(shape)
    _, gv, _ = run(gpu, maps, u.verts, u.vert_mesh, cameras(gpu), g, maps_want_grad, headroom, monkeypatch)
    assert gv.shape == (u.vt, 3)
    for m, ref in enumerate(reference(gpu, shape)):
        if ref is not None:
            assert torch.equal(gv[u.vids[m].to(gpu)], ref[1]), "mesh %d" % m
            assert float(ref[1].abs().max()) > 0


# ---------------------------------------------------------------- 3: the position gradient against float64
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_position_gradient_against_float64(gpu, shape):
    """Per mesh, with the fp32 cameras actually used.  Vertices left out (within 1e-3 texels of a texel line), from the float64
    restatement alone: four-map 0 / 1 / 0, two-map 1 / 0 / 0, dims (14, 7) 1 / 0 / 1, training shape 1 / 1 / 1 of 101 / 101 / 70
    -- the helper's 2 % cap is a condition and holds.  The outer shell of meshes 0 and 1 is clamped on both axes for some
    vertices: exactly zero rows."""
    u = union()
    maps, g = maps_and_gradient(shape)
    cams = cameras(gpu)
    _, gv, _ = run(gpu, maps, u.verts, u.vert_mesh, cams, g)
    for m in range(3):
        ids = u.vids[m]
        r = pool_vertex_gradient_close(gv[ids.to(gpu)][None], [t[m:m + 1] for t in maps], u.local[m][None], cams[0][m:m + 1], cams[1][m:m + 1],
                                       g[ids][None], "ragged pooling verts.grad %s mesh %d" % (shape, m))
        assert r["live_rows"] >= 50, r
        if m < 2:
            assert r["zero_rows"] >= 9 and r["zero_checked"] >= r["zero_rows"] - 1, r


# ---------------------------------------------------------------- 4: the map gradient, every element against float64
@pytest.mark.parametrize("shape", ("four_maps", "training"))
def test_map_gradient_per_element_against_float64(gpu, shape):
    """The pooling is linear in the maps: pooling identity maps (channel t = the one-hot map of texel t) returns P with the
    weights as the kernel forms them (ragged_pooling itself, pinned bit for bit above), and the gradient of mesh m's map is
    P_m^T g_m in float64, bound 8 eps * sum |P||g| per element.  Mesh 3 has no vertices: its gradient is written, as zeros; so is
    every texel nothing projects into."""
    u = union()
    chans, dims = SHAPES[shape]
    maps, g = maps_and_gradient(shape)
    cams = cameras(gpu)
    _, _, gmaps = run(gpu, maps, u.verts, u.vert_mesh, cams, g)
    verts, ids, gd = u.verts.to(gpu), u.vert_mesh.to(gpu), g.to(gpu).double()
    col = 0
    for c, d, got in zip(chans, dims, gmaps):
        assert got.shape == (B, c, d, d)
        eye = torch.eye(d * d, device=gpu).view(1, d * d, d, d).expand(B, -1, -1, -1).contiguous()
        P = utils.ragged_pooling([eye], verts, ids, cams).double()                                   # [Vt, d*d]
        del eye
        gl = gd[:, col:col + c]
        for m in range(B):
            mine = ids == m
            ref = torch.einsum("vt,vc->ct", P[mine], gl[mine]).view(c, d, d)
            bound = 8 * EPS * torch.einsum("vt,vc->ct", P[mine].abs(), gl[mine].abs()).view(c, d, d) + 1e-30
            err = (got[m].double() - ref).abs()
            assert bool((err <= bound).all()), "map %d x %d mesh %d: err/bound up to %.3g" % (d, d, m, float((err / bound).max()))
            assert bool((got[m][ref == 0] == 0).all())
            if m < 3 and d > 1:         # (a 1 x 1 map: the coordinate is integral, all four weights are zero)
                assert float(ref.abs().max()) > 0 and (bool((ref == 0).any()) or d < 28)
        assert bool((got[3] == 0).all())
        col += c


# ---------------------------------------------------------------- 5: ids outside the batch
@pytest.mark.parametrize("shape", ("four_maps", "wide"))
def test_a_vertex_whose_id_is_outside_the_batch_belongs_to_no_mesh(gpu, shape):
    u = union()
    maps, g = maps_and_gradient(shape)
    cams = cameras(gpu)
    ids = u.vert_mesh.clone()
    stray = [int(u.vids[0][3]), int(u.vids[2][0])]
    ids[stray[0]], ids[stray[1]] = -1, B
    feats, gv, gmaps = run(gpu, maps, u.verts, ids, cams, g)
    assert bool((feats[stray] == 0).all()) and bool((gv[stray] == 0).all())
    keep = torch.ones(u.vt, dtype=torch.bool)
    keep[stray] = False
    f2, gv2, gmaps2 = run(gpu, maps, u.verts[keep], ids[keep], cams, g[keep])
    assert torch.equal(feats[keep.to(gpu)], f2) and torch.equal(gv[keep.to(gpu)], gv2)
    assert float(f2.abs().max()) > 0 and float(gv2.abs().max()) > 0
    for a, b in zip(gmaps, gmaps2):
        close_in_list_order(a, b, "map gradient with and without the stray rows")
    # ... and far outside, through int64: still no mesh, nothing indexed
    ids[stray[0]], ids[stray[1]] = -(2 ** 40), 2 ** 33 + 1
    f3, gv3, gmaps3 = run(gpu, maps, u.verts, ids, cams, g)
    assert torch.equal(f3, feats) and torch.equal(gv3, gv)
    for a, b in zip(gmaps3, gmaps):
        close_in_list_order(a, b, "map gradient with far ids")


# ---------------------------------------------------------------- 6: the forward's row pitch through the C ABI
def test_forward_writes_pitched_rows_through_the_c_abi(gpu):
    u = union()
    chans, dims = SHAPES["four_maps"]
    maps, _ = maps_and_gradient("four_maps")
    cam_mat, cam_pos = cameras(gpu)
    blks = [t.to(gpu) for t in maps]
    verts, vert_mesh = u.verts.to(gpu), u.vert_mesh.to(gpu)
    want = utils.ragged_pooling(blks, verts, vert_mesh, (cam_mat, cam_pos))
    ids32, _ = ragged.mesh_counts(vert_mesh, B)
    vert_list, _ = ragged.group_vertices(vert_mesh, B)
    ctot, n = sum(chans), len(chans)
    buf = torch.full((u.vt, ctot + 5), -7.25, device=gpu)
    _lib.call("geom_pool_features_ragged_fwd_f32", B, u.vt, verts, ids32, vert_list, cam_mat, cam_pos, n, blks, (ctypes.c_int * n)(*chans),
              (ctypes.c_int * n)(*dims), buf[:, 5:], ctot + 5)
    assert torch.equal(buf[:, 5:], want)
    assert bool((buf[:, :5] == -7.25).all())


# ---------------------------------------------------------------- 7: NaN and Inf travel as in the batched launches
@pytest.mark.parametrize("what", ("nan_position", "inf_map", "nan_camera"))
def test_non_finite_values_travel_as_in_the_batched_launches(gpu, what):
    """The ragged instantiations share the bodies: features and both gradients against the per-mesh
    batched calls on the same non-finite inputs -- the NaN masks agree and everything else is equal (map gradients: in list
    order, see the module's docstring)."""
    u = union()
    maps, g = maps_and_gradient("four_maps")
    maps = [t.clone() for t in maps]
    verts, local = u.verts.clone(), [t.clone() for t in u.local]
    cam_mat, cam_pos = (t.clone() for t in cameras(gpu))
    if what == "nan_position":
        local[1][17, 1] = float("nan")
        verts[u.vids[1][17]] = local[1][17]
    elif what == "inf_map":
        maps[2][0, 5, 20, 21] = float("inf")
        maps[1][2, 3] = float("-inf")
    else:
        cam_pos[2, 0] = float("nan")
    feats, gv, gmaps = run(gpu, maps, verts, u.vert_mesh, (cam_mat, cam_pos), g)
    refs = per_mesh(gpu, maps, local, (cam_mat, cam_pos), [g[ids] for ids in u.vids])
    # a vertex whose projection is NaN sits at texel 0 with four zero weights -- its row is 0 * texel 0, its
    # verts.grad row exactly zero (the clamp is a select) --, so only a non-finite MAP value shows in the result
    if what == "inf_map":
        assert not bool(torch.isfinite(feats).all())
    else:
        hit = [int(u.vids[1][17])] if what == "nan_position" else u.vids[2].tolist()
        assert bool((feats[hit] == 0).all()) and bool((gv[hit] == 0).all())
    for m, ref in enumerate(refs):
        if ref is None:
            continue
        ids = u.vids[m].to(gpu)
        assert same_with_nan(feats[ids], ref[0]), "features of mesh %d" % m
        assert same_with_nan(gv[ids], ref[1]), "position gradient of mesh %d" % m
        for got, want in zip(gmaps, ref[2]):
            close_in_list_order(got[m:m + 1], want, "map gradient of mesh %d" % m)
    for got in gmaps:
        assert bool((got[3] == 0).all())


# ---------------------------------------------------------------- 8: graph capture
def test_forward_and_backward_replay_from_a_captured_graph(gpu):
    """No host read once the grouping is cached: forward + backward captured in one graph after a warm-up call, replayed on new
    positions copied into the captured tensor, against the eager call on those positions."""
    u = union()
    maps, g = maps_and_gradient("four_maps")
    cams = cameras(gpu)
    ids = u.vert_mesh.to(gpu)
    v = u.verts.to(gpu).requires_grad_(True)
    mm = [t.to(gpu).requires_grad_(True) for t in maps]
    gd = g.to(gpu)

    def step():
        feats = utils.ragged_pooling(mm, v, ids, cams)
        return (feats,) + torch.autograd.grad(feats, [v] + mm, gd)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                   # fills the caches (the grouping, the ids, the binding)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    moved = (u.verts * 0.97 + 0.004).to(gpu)
    with torch.no_grad():
        v.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    feats, gv, gmaps = run(gpu, maps, moved, u.vert_mesh, cams, g)
    first = run(gpu, maps, u.verts, u.vert_mesh, cams, g)
    assert not torch.equal(first[0], feats)                       # the replay did see the new positions
    assert torch.equal(captured[0], feats) and torch.equal(captured[1], gv)
    for a, b in zip(captured[2:], gmaps):
        close_in_list_order(a, b, "map gradient from the replay")


# ---------------------------------------------------------------- 9: two runs, the same bits
@pytest.mark.parametrize("shape", ("wide", "training"))
def test_features_and_position_gradient_are_bit_reproducible(gpu, shape):
    """The per-chunk sums are added in chunk order whatever order the workgroups finished in (40 chunks on 32 grid slices, and
    the training shape).  The map gradient's bits are NOT asserted: the order inside a texel's list follows an atomic cursor, as
    in the batched launch, so its fp32 summation order may differ between two runs."""
    u = union()
    maps, g = maps_and_gradient(shape)
    cams = cameras(gpu)
    first = run(gpu, maps, u.verts, u.vert_mesh, cams, g)
    again = run(gpu, maps, u.verts, u.vert_mesh, cams, g)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert float(first[1].abs().max()) > 0
    for a, b in zip(first[2], again[2]):
        close_in_list_order(a, b, "map gradient of two runs")
