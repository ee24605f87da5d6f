"""-m gpu: the projection-matrix pooling (csrc/pooling.hip's bodies instantiated for MX = true by
csrc/pooling_proj.hip) -- utils.pooling(blocks, verts_pos, matrix), and batched_pooling / ragged_pooling given an fp32 [B,4,4]
tensor -- on the union of test_ragged_pooling_gpu.py: 101, 101, 70 and 0 vertices, 272 rows interleaved by a seeded permutation
(all five 64-position tiles of the grouped list, two of them straddling a mesh boundary), at its four shapes.

Matrices (tests/pool_matrix_ref.py): family E, equivalent to the cameras (35, 20, 1.2), (250, -30, 0.8), (60, 30, 1.0), and G, E
with every entry perturbed by up to 3 % and row 2 = 1e30; the empty mesh 3 gets a fourth matrix nothing projects with.

What the kernels are held to, in this order: the float64 restatement pool_matrix_ref (pinned on the host to the reference's own
float64 run), the reference's fp32 run stored in tests/golden/pooling_matrix.npz, and -- ragged and batched against the b = 1
calls -- their own bits.  Bounds:
  * position gradient: pool_matrix_ref.vertex_gradient_close -- helpers.POOL_ROW_RTOL (8 eps) of the element's term mass + 1
    texel-coordinate ulp through every term, vertices within 1e-3 texels of a texel line left out under the 2 % cap, exactly zero
    rows where float64 is exactly zero;
  * map gradient: every element against P^T g in float64 at 8 eps * sum |P||g|, P = the kernel's own weights (identity maps
    pooled), which are held to float64 on their own:
  * projection and weights: POOL_MATRIX_P_ULPS = 3.9 eps * dim = 4 x the 0.975 the restatement's own fp32 host run reaches on
    the kept vertices (measured, test_matrix_pooling_host.py re-measures it).
  * a map gradient against another launch's: LIST_ORDER_RTOL = 2e-6 of the tensor's largest entry (the order inside a texel's
    list follows an atomic cursor in both).  For the same reason a map gradient is never compared bit for bit, whatever is.

Measured on the MI355X (GEOM_MARGIN_LOG), worst element as a share of its bound, the restatement's own fp32 host run in
brackets where it was measured: position gradient against float64 0.065 (E, two_maps, mesh 0) [0.066 on the same case; 0.233 at
the worst on the fixture's thin shape], features 0.195, map gradient 0.216 (E, wide, 14 x 14), P 0.975 eps * dim = 0.25 of the
bar [0.975: the kernel evaluates the restatement's expressions in its order]; against the reference's fp32 run: position
gradient 0.272, features 0.165, map gradient 0.222; matrix against camera route: position gradient 0.055, features 0.138."""
import functools

import numpy as np
import pytest
import torch

import pool_matrix_ref as pm
from helpers import golden, log_margin
from geometrics_amd import ops, utils
from oracle import ref_ops
from test_pooling_vertex_gradient_gpu import POOL_P_ULPS
from test_ragged_pooling_gpu import B, LIST_ORDER_RTOL, SHAPES, close_in_list_order, maps_and_gradient, union

pytestmark = pytest.mark.gpu

EPS = pm.EPS
FIXTURE_CASES = [(f, m, "thin") for f in "EG" for m in range(3)] + [("G", 1, "two_maps")]
assert LIST_ORDER_RTOL == 2e-6


@functools.lru_cache(maxsize=None)
def matrices(fam):
    """[4,4,4] fp32 (host): the family's three matrices and, for the empty mesh, the first one scaled."""
    three = pm.family(fam)[0]
    return torch.cat((three, 1.25 * three[:1]))


# ---------------------------------------------------------------- the b = 1 calls, computed once per (family, shape) and shared
def single(gpu, maps_m, verts, matrix, grad_rows, maps_want_grad=True):
    """utils.pooling for ONE mesh on the device: (features [V,C], verts.grad [V,3], [map gradients [c,d,d]] or None)."""
    v = verts.to(gpu).requires_grad_(True)
    mm = [t.to(gpu).requires_grad_(maps_want_grad) for t in maps_m]
    feats = utils.pooling(mm, v, matrix.to(gpu))
    got = torch.autograd.grad(feats, [v] + (mm if maps_want_grad else []), grad_rows.to(gpu))
    return feats.detach(), got[0], list(got[1:]) if maps_want_grad else None


_per_mesh = {}


def per_mesh(gpu, fam, shape):
    if (fam, shape) not in _per_mesh:
        u = union()
        maps, g = maps_and_gradient(shape)
        _per_mesh[fam, shape] = [single(gpu, [t[m] for t in maps], u.local[m], matrices(fam)[m], g[u.vids[m]]) for m in range(3)]
    return _per_mesh[fam, shape]


def run(gpu, maps, verts, vert_mesh, proj, grad_out, maps_want_grad=True, headroom=0, monkeypatch=None):
    """utils.ragged_pooling with matrices, forward and backward -> (features, verts.grad, [map gradients] or None).  headroom:
    grad_out handed in as the trailing columns of a buffer that much wider; the pitch the backward launch received is checked."""
    v = verts.to(gpu).requires_grad_(True)
    mm = [t.to(gpu).requires_grad_(maps_want_grad) for t in maps]
    feats = utils.ragged_pooling(mm, v, vert_mesh.to(gpu), proj.to(gpu))
    ctot = grad_out.shape[1]
    wide = torch.zeros(grad_out.shape[0], headroom + ctot, device=gpu)
    wide[:, headroom:] = grad_out.to(gpu)
    pitches, call = [], ops._lib.call

    def recording_call(name, *args):
        assert name != "geom_pool_features_ragged_bwd_f32"                  # (the camera route is not this one)
        if name == "geom_pool_features_ragged_proj_bwd_f32":
            pitches.append(int(args[12]))                                   # grad_ld (0 = the pooled width)
        return call(name, *args)

    if monkeypatch is not None:
        monkeypatch.setattr(ops._lib, "call", recording_call)
    got = torch.autograd.grad(feats, [v] + (mm if maps_want_grad else []), wide[:, headroom:])
    if monkeypatch is not None:
        monkeypatch.setattr(ops._lib, "call", call)
        assert pitches == [headroom + ctot if headroom else 0]
    return feats.detach(), got[0], list(got[1:]) if maps_want_grad else None


def kernel_operator(gpu, verts, matrix, d):
    """P [V, d*d] as the kernel forms it: the identity maps of ONE image pooled by utils.pooling."""
    return utils.pooling([torch.eye(d * d, device=gpu).view(d * d, d, d)], verts.to(gpu), matrix.to(gpu))


def map_gradients_close(gpu, gmaps, chans, dims, verts, matrix, g_rows, what):
    """Every element of one mesh's map gradients [c,d,d] against P^T g in float64 (P: the kernel's), 8 eps * sum |P||g|; a texel
    nothing projects into is exactly zero."""
    col, worst = 0, 0.0
    for c, d, got in zip(chans, dims, gmaps):
        assert got.shape == (c, d, d)
        P = kernel_operator(gpu, verts, matrix, d).double().cpu()
        gl = g_rows[:, col:col + c].double()
        col += c
        ref = torch.einsum("vt,vc->ct", P, gl)
        share = pm.map_gradient_share(got, ref, P, gl, d, None)
        assert log_margin("%s map %d x %d" % (what, d, d), share, 1.0), "%s map %d x %d: err/bound %.3g" % (what, d, d, share)
        assert bool((got.cpu().view(c, -1)[:, P.abs().sum(0) == 0] == 0).all())
        worst = max(worst, share)
    return worst


# ---------------------------------------------------------------- 1: utils.pooling per mesh against float64
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fam", ("E", "G"))
def test_pooling_per_mesh_against_float64(gpu, fam, shape):
    """Position gradient element by element and every element of the map gradients, per mesh.  Host figures (the restatement's
    own fp32 run, share of the position-gradient bound): 0.233 at the worst (G, mesh 1, thin shape of the fixture)."""
    u = union()
    chans, dims = SHAPES[shape]
    maps, g = maps_and_gradient(shape)
    for m, (feats, gv, gmaps) in enumerate(per_mesh(gpu, fam, shape)):
        what = "matrix pooling %s %s mesh %d" % (fam, shape, m)
        rows, M = g[u.vids[m]], matrices(fam)[m]
        assert feats.shape == (u.sizes[m], sum(chans)) and gv.shape == (u.sizes[m], 3)
        r = pm.vertex_gradient_close(gv[None], [t[m:m + 1] for t in maps], u.local[m][None], M[None], rows[None], what + " verts.grad")
        assert r["live_rows"] >= 50, r
        if m < 2:       # the outer shell: clamped on both axes of every map for some vertices -- exactly zero rows
            assert r["zero_rows"] >= 6 and r["zero_checked"] >= r["zero_rows"] - 1, r
        map_gradients_close(gpu, gmaps, chans, dims, u.local[m], M, rows, what)
        err = (feats.double().cpu() - pm.pool_features([t[m:m + 1].double() for t in maps], u.local[m][None].double(), M[None].double())[0]).abs()
        share = (err / (pm.feature_bound([t[m:m + 1] for t in maps], u.local[m][None], M[None])[0] + 1e-30))[torch.from_numpy(r["keep"][0])]
        assert log_margin(what + " features", float(share.max()), 1.0), float(share.max())


@pytest.mark.parametrize("group", (0, 1), ids=("ragged_dims", "training_dims"))
@pytest.mark.parametrize("fam", ("E", "G"))
def test_projection_and_weights_against_float64(gpu, fam, group):
    """The kernel's P against the restatement's float64 P per element on the kept vertices: which texels a vertex reads and with
    which weights.  The bar is measured, not chosen: POOL_MATRIX_P_ULPS = 3.9 eps * dim = 4 x the worst the restatement's own fp32
    host run reaches (0.975, at 9 x 9, G on mesh 1).  The kernel on the MI355X reaches 0.975 as well, at the same place (G, the
    ragged shapes' maps): 0.25 of the bar -- a margin of 4, as the bar was made."""
    u = union()
    dims = pm.P_DIMS[group]
    worst = 0.0
    for m in range(3):
        verts, M = u.local[m], matrices(fam)[m]
        keep = pm.kept_vertices(verts[None], M[None], dims)
        for d in dims:
            worst = max(worst, pm.weights_error(kernel_operator(gpu, verts, M, d)[None], verts[None], M[None], d, keep))
    assert log_margin("matrix pooling P %s %s (eps * dim)" % (fam, dims), worst, pm.POOL_MATRIX_P_ULPS), "the kernel's weights are %.2f eps * dim off" % worst


# ---------------------------------------------------------------- 2: the fixture cases against the reference's own fp32 results
@pytest.mark.parametrize("fam, m, shape", FIXTURE_CASES)
def test_fixture_cases_against_the_reference_fp32_run(gpu, fam, m, shape):
    """Two fp32 evaluations held to each other under the bound ONE of them gets against float64 (the reference forms q with
    torch.mm: its bits are not the target).  The map gradient: the reference's weights are its own, so the bound carries the P
    bar and the texels around a left-out vertex are not compared (pool_matrix_ref.map_gradient_share)."""
    g = golden("pooling_matrix")
    key = "%s.m%d.%s" % (fam, m, shape)
    verts, proj = torch.from_numpy(g[key + ".verts"]), torch.from_numpy(g[key + ".proj"])
    maps, cot = pm.maps_and_gradient(shape, verts.shape[0])
    chans, dims = pm.SHAPES[shape]
    feats, gv, gmaps = single(gpu, [t[0] for t in maps], verts, proj, cot[0])
    r = pm.vertex_gradient_close(gv[None], maps, verts[None], proj[None], cot, "kernel against the reference fp32 verts.grad " + key,
                                 against=g[key + ".gv32"][None])
    keep = torch.from_numpy(r["keep"][0])
    err = (feats.double().cpu() - torch.from_numpy(g[key + ".feats32"]).double()).abs()
    share = (err / (pm.feature_bound(maps, verts[None], proj[None])[0] + 1e-30))[keep]
    assert log_margin("kernel against the reference fp32 features " + key, float(share.max()), 1.0), float(share.max())
    col = 0
    for l, (c, d) in enumerate(zip(chans, dims)):
        P = pm.pool_operator(verts[None].double(), proj[None].double(), d)[0]
        share = pm.map_gradient_share(gmaps[l], g["%s.gm32.%d" % (key, l)], P, cot[0, :, col:col + c], d, keep, pm.POOL_MATRIX_P_ULPS)
        col += c
        assert log_margin("kernel against the reference fp32 gradient of map %d %s" % (l, key), share, 1.0), share


# ---------------------------------------------------------------- 3: ragged_pooling with [B,4,4] against utils.pooling per mesh
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fam", ("E", "G"))
def test_ragged_features_equal_the_per_mesh_calls_bit_for_bit(gpu, fam, shape):
    u = union()
    maps, _ = maps_and_gradient(shape)
    feats = utils.ragged_pooling([t.to(gpu) for t in maps], u.verts.to(gpu), u.vert_mesh.to(gpu), matrices(fam).to(gpu))
    assert feats.shape == (u.vt, sum(SHAPES[shape][0])) and feats.is_contiguous()
    for m, ref in enumerate(per_mesh(gpu, fam, shape)):
        assert torch.equal(feats[u.vids[m].to(gpu)], ref[0]), "mesh %d" % m
        assert float(ref[0].abs().max()) > 0
    again = utils.ragged_pooling([t.to(gpu) for t in maps], u.verts.to(gpu), u.vert_mesh.to(gpu, torch.int32), matrices(fam).to(gpu))
    assert torch.equal(again, feats)


@pytest.mark.parametrize("maps_want_grad", (True, False), ids=("with_maps", "verts_only"))
@pytest.mark.parametrize("headroom", (0, 7))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_ragged_gradients_equal_the_per_mesh_ones(gpu, monkeypatch, shape, headroom, maps_want_grad):
    """Position gradient bit for bit, the gradient contiguous and pitched, with and without map gradients; map gradients in list
    order; the empty mesh's map gradient is written, as zeros.  (Family G: all twelve used entries general.)"""
    u = union()
    maps, g = maps_and_gradient(shape)
    _, gv, gmaps = run(gpu, maps, u.verts, u.vert_mesh, matrices("G"), g, maps_want_grad, headroom, monkeypatch)
    assert gv.shape == (u.vt, 3)
    for m, ref in enumerate(per_mesh(gpu, "G", shape)):
        assert torch.equal(gv[u.vids[m].to(gpu)], ref[1]), "mesh %d" % m
        assert float(ref[1].abs().max()) > 0
        if maps_want_grad:
            for got, want in zip(gmaps, ref[2]):
                close_in_list_order(got[m], want, "map gradient of mesh %d" % m)
    if maps_want_grad:
        for got in gmaps:
            assert bool((got[3] == 0).all())


@pytest.mark.parametrize("shape", ("four_maps", "wide"))
def test_a_vertex_whose_id_is_outside_the_batch_belongs_to_no_mesh(gpu, shape):
    u = union()
    maps, g = maps_and_gradient(shape)
    proj = matrices("G")
    ids = u.vert_mesh.clone()
    stray = [int(u.vids[0][3]), int(u.vids[2][0])]
    ids[stray[0]], ids[stray[1]] = -1, B
    feats, gv, gmaps = run(gpu, maps, u.verts, ids, proj, g)
    assert bool((feats[stray] == 0).all()) and bool((gv[stray] == 0).all())
    keep = torch.ones(u.vt, dtype=torch.bool)
    keep[stray] = False
    f2, gv2, gmaps2 = run(gpu, maps, u.verts[keep], ids[keep], proj, g[keep])
    assert torch.equal(feats[keep.to(gpu)], f2) and torch.equal(gv[keep.to(gpu)], gv2)
    assert float(f2.abs().max()) > 0 and float(gv2.abs().max()) > 0
    for a, b in zip(gmaps, gmaps2):
        close_in_list_order(a, b, "map gradient with and without the stray rows")
    ids[stray[0]], ids[stray[1]] = -(2 ** 40), 2 ** 33 + 1                  # far outside, through int64: still no mesh
    f3, gv3, _ = run(gpu, maps, u.verts, ids, proj, g)
    assert torch.equal(f3, feats) and torch.equal(gv3, gv)


# ---------------------------------------------------------------- 4: batched_pooling with [3,4,4]
@pytest.mark.parametrize("shape", ("four_maps", "training"))
def test_batched_pooling_with_matrices_equals_the_three_single_calls(gpu, monkeypatch, shape):
    """Three meshes of 70 vertices each: bit for bit the b = 1 calls (features, position gradient); with headroom= / fronts= the
    plain call's bits, the fronts in place; the pitch handed to the backward launch is checked."""
    u = union()
    maps, g = maps_and_gradient(shape)
    ctot = g.shape[1]
    verts = torch.stack([u.local[m][:70] for m in range(3)])
    grad = torch.stack([g[u.vids[m][:70]] for m in range(3)])
    proj = matrices("G")[:3]
    mm = [t[:3].to(gpu).contiguous().requires_grad_(True) for t in maps]
    v = verts.to(gpu).requires_grad_(True)
    feats = utils.batched_pooling(mm, v, proj.to(gpu))
    assert feats.shape == (3, 70, ctot)
    got = torch.autograd.grad(feats, [v] + mm, grad.to(gpu))
    for m in range(3):
        f1, gv1, gm1 = single(gpu, [t[m] for t in maps], verts[m], proj[m], grad[m])
        assert torch.equal(feats[m], f1) and torch.equal(got[0][m], gv1), "mesh %d" % m
        for a, b in zip(got[1:], gm1):
            close_in_list_order(a[m], b, "map gradient of mesh %d" % m)
    # headroom and fronts: the features as the trailing columns of a wider buffer, the fronts copied in front by the same launch
    prev, front = torch.randn(3, 70, 5, generator=torch.Generator().manual_seed(3)).to(gpu), verts.to(gpu)
    v2 = verts.to(gpu).requires_grad_(True)
    wide = utils.batched_pooling(mm, v2, proj.to(gpu), headroom=8, fronts=(front, prev))
    assert torch.equal(wide, feats.detach()) and ops.headroom_of(wide) == 8
    rec = ops.wide_buffer_of(wide)
    assert rec.buf is not None and rec.buf.shape == (3, 70, 8 + ctot) and rec.holds(0, front) and rec.holds(3, prev)
    assert torch.equal(rec.buf[..., :3], front) and torch.equal(rec.buf[..., 3:8], prev)
    assert torch.equal(utils.batched_pooling(mm, v2, proj.to(gpu), headroom=8), feats.detach())           # headroom alone
    pitches, call = [], ops._lib.call

    def recording_call(name, *args):
        if name == "geom_pool_features_proj_bwd_f32":
            pitches.append(int(args[9]))                                    # grad_ld (0 = the pooled width)
        return call(name, *args)

    monkeypatch.setattr(ops._lib, "call", recording_call)
    cot = torch.zeros(3, 70, 8 + ctot, device=gpu)
    cot[..., 8:] = grad.to(gpu)
    gv2 = torch.autograd.grad(wide, [v2], cot[..., 8:])[0]                    # the gradient read pitched, in place
    monkeypatch.setattr(ops._lib, "call", call)
    assert pitches == [8 + ctot]
    assert torch.equal(gv2, got[0])


# ---------------------------------------------------------------- 5: row 2 is never read
def test_row_2_of_the_matrix_is_never_read(gpu):
    """Row 2 replaced by NaN: the features and the position gradient are the clean run's bits, the map gradients the clean run's in
    list order (and hold no NaN) -- ragged, batched at b = 1 (utils.pooling) alike."""
    u = union()
    maps, g = maps_and_gradient("four_maps")
    clean, poisoned = matrices("E").clone(), matrices("E").clone()
    clean[:, 2] = 0.0
    poisoned[:, 2] = float("nan")
    a, b = run(gpu, maps, u.verts, u.vert_mesh, clean, g), run(gpu, maps, u.verts, u.vert_mesh, poisoned, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[1].abs().max()) > 0
    for x, y in zip(a[2], b[2]):
        assert bool(torch.isfinite(y).all())
        close_in_list_order(y, x, "map gradient with row 2 = NaN")
    a = single(gpu, [t[1] for t in maps], u.local[1], clean[1], g[u.vids[1]])
    b = single(gpu, [t[1] for t in maps], u.local[1], poisoned[1], g[u.vids[1]])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], per_mesh(gpu, "E", "four_maps")[1][0])         # (and row 2 = 0 is family E itself)


# ---------------------------------------------------------------- 6: with E, the matrix route against the camera route
@pytest.mark.parametrize("shape", ("four_maps", "two_maps"))
def test_with_equivalent_matrices_the_camera_route_is_the_yardstick(gpu, shape):
    """The EXISTING camera route (utils.batched_pooling with the fp32 cameras of batch_camera_info) and the matrix route with the
    matrices equivalent to those cameras (rounded to fp32), on the kept vertices: they differ by no more than the sum of their two
    float64 bounds -- each against ITS float64 restatement with ITS fp32 inputs -- plus what those two float64 values differ by
    (the rounding of the matrices' entries; computed in float64, not granted)."""
    u = union()
    chans, dims = SHAPES[shape]
    maps, g = maps_and_gradient(shape)
    cam_mat, cam_pos = utils.batch_camera_info(torch.tensor(pm.CAMERAS).to(gpu))
    E = pm.equivalent_matrices(cam_mat.cpu(), cam_pos.cpu()).float()
    for m in range(3):
        verts, rows, mm = u.local[m], g[u.vids[m]], [t[m:m + 1] for t in maps]
        fm, gvm, _ = single(gpu, [t[m] for t in maps], verts, E[m], rows)
        v = verts.to(gpu)[None].requires_grad_(True)
        fc = utils.batched_pooling([t.to(gpu) for t in mm], v, (cam_mat[m:m + 1].contiguous(), cam_pos[m:m + 1].contiguous()))
        gvc = torch.autograd.grad(fc, [v], rows.to(gpu)[None])[0][0]
        cm, cp = cam_mat[m:m + 1].cpu(), cam_pos[m:m + 1].cpu()
        grad_m, mass_m, floor_m, near_m = pm.pool_vertex_gradient(mm, verts[None], E[m][None], rows[None])
        grad_c, mass_c, floor_c, near_c = ref_ops.pool_vertex_gradient(mm, verts[None], cm, cp, rows[None])
        keep = (near_m[0] >= 1e-3) & (near_c[0] >= 1e-3)
        assert (~keep).mean() <= 0.02
        bound = 8 * EPS * (mass_m + mass_c)[0] + (floor_m + floor_c)[0] + np.abs(grad_m - grad_c)[0] + 1e-30
        share = (np.abs(gvm.double().cpu().numpy() - gvc.double().cpu().numpy()) / bound)[keep]
        assert log_margin("matrix against camera route verts.grad %s mesh %d" % (shape, m), float(share.max()), 1.0), float(share.max())
        f64_m = pm.pool_features([t.double() for t in mm], verts[None].double(), E[m][None].double())[0]
        f64_c = ref_ops.pool_features([t.double() for t in mm], verts[None].double(), cm.double(), cp.double())[0]
        bound = pm.feature_bound(mm, verts[None], E[m][None])[0] + pm.feature_bound(mm, verts[None], E[m][None], POOL_P_ULPS)[0] \
            + (f64_m - f64_c).abs() + 1e-30
        share = ((fm.double().cpu() - fc[0].detach().double().cpu()).abs() / bound)[torch.from_numpy(keep)]
        assert log_margin("matrix against camera route features %s mesh %d" % (shape, m), float(share.max()), 1.0), float(share.max())
        assert float((fm - fc[0].detach()).abs().max()) < 1e-3 * float(fc.detach().abs().max())      # (they ARE the same projection)


# ---------------------------------------------------------------- 7: non-finite values (the pooling rule)
@pytest.mark.parametrize("what", ("nan_position", "nan_matrix_row_0", "q3_zero"))
def test_non_finite_values_follow_the_pooling_rule(gpu, what):
    """A NaN projection lands at texel 0 with zero weights on its axis: the feature row is 0 (finite maps) and the verts.grad row
    exactly zero; q3 == 0 with q0 != 0 is an infinite coordinate, which the clamp holds like any far point (an integral
    coordinate: zero weights, nothing through the clamp).  The affected rows are the restatement's fp32 host run's, every other
    row is the clean run's bit for bit, and the map gradients are P^T g of the kernel's own weights."""
    u = union()
    shape = "four_maps"
    chans, dims = SHAPES[shape]
    maps, g = maps_and_gradient(shape)
    proj = matrices("G").clone()
    proj[2, 3] = torch.tensor([0.0, 0.0, 1.0, 0.0])                          # mesh 2: q3 = z exactly
    verts, local = u.verts.clone(), [t.clone() for t in u.local]
    clean = run(gpu, maps, verts, u.vert_mesh, proj, g)
    planted = proj.clone()
    if what == "nan_position":
        local[1][17, 1] = float("nan")
        verts[u.vids[1][17]] = local[1][17]
        hit = [int(u.vids[1][17])]
    elif what == "nan_matrix_row_0":
        planted[1, 0, 2] = float("nan")
        hit = u.vids[1].tolist()
    else:
        local[2][5, 2] = 0.0
        verts[u.vids[2][5]] = local[2][5]
        hit = [int(u.vids[2][5])]
        q0, _, q3, _, _ = pm.project(local[2][None], planted[2][None])
        assert float(q3[0, 5]) == 0.0 and float(q0[0, 5]) != 0.0
    feats, gv, gmaps = run(gpu, maps, verts, u.vert_mesh, planted, g)
    others, hit_set = torch.ones(u.vt, dtype=torch.bool), set(hit)
    others[hit] = False
    assert torch.equal(feats[others.to(gpu)], clean[0][others.to(gpu)]) and torch.equal(gv[others.to(gpu)], clean[1][others.to(gpu)])
    assert bool((feats[hit] == 0).all()) and bool((gv[hit] == 0).all())
    for m in range(3):
        mm = [t[m:m + 1] for t in maps]
        host = pm.pool_features(mm, local[m][None], planted[m][None])[0]                  # the restatement's fp32 host run
        mine = torch.tensor([i for i, v in enumerate(u.vids[m].tolist()) if v in hit_set], dtype=torch.long)
        assert torch.equal(feats[u.vids[m].to(gpu)].cpu()[mine], host[mine])
        grad64 = pm.pool_vertex_gradient(mm, local[m][None], planted[m][None], g[u.vids[m]][None])[0][0]
        assert (grad64[mine.numpy()] == 0).all()
        map_gradients_close(gpu, [t[m] for t in gmaps], chans, dims, local[m], planted[m], g[u.vids[m]], "%s mesh %d" % (what, m))
    for got in gmaps:
        assert bool(torch.isfinite(got).all()) and bool((got[3] == 0).all())
        if what == "nan_matrix_row_0":
            assert bool((got[1] == 0).all())                                 # every vertex of mesh 1: four zero weights


# ---------------------------------------------------------------- 8: graph capture, and two runs
def test_forward_and_backward_replay_from_a_captured_graph(gpu):
    """Forward + backward of the ragged matrix route captured in one graph after a warm-up; the replay on new positions, maps and
    matrices (copied into the captured tensors) gives the eager bits; two eager runs give the same features and position gradient."""
    u = union()
    maps, g = maps_and_gradient("four_maps")
    ids = u.vert_mesh.to(gpu)
    v = u.verts.to(gpu).requires_grad_(True)
    mm = [t.to(gpu).requires_grad_(True) for t in maps]
    proj = matrices("E").to(gpu)
    gd = g.to(gpu)

    def step():
        feats = utils.ragged_pooling(mm, v, ids, proj)
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
    moved = u.verts * 0.97 + 0.004
    maps2 = [t * 1.5 - 0.25 for t in maps]
    with torch.no_grad():
        v.copy_(moved.to(gpu))
        proj.copy_(matrices("G").to(gpu))
        for t, s in zip(mm, maps2):
            t.copy_(s.to(gpu))
    graph.replay()
    torch.cuda.synchronize()
    feats, gv, gmaps = run(gpu, maps2, moved, u.vert_mesh, matrices("G"), g)
    first = run(gpu, maps, u.verts, u.vert_mesh, matrices("E"), g)
    assert not torch.equal(first[0], feats)                       # the replay did see the new inputs
    assert torch.equal(captured[0], feats) and torch.equal(captured[1], gv)
    for a, b in zip(captured[2:], gmaps):
        close_in_list_order(a, b, "map gradient from the replay")
    again = run(gpu, maps2, moved, u.vert_mesh, matrices("G"), g)
    assert torch.equal(again[0], feats) and torch.equal(again[1], gv) and float(gv.abs().max()) > 0
