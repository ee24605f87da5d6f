"""-m gpu: the surface loss of a RAGGED batch -- meshes with their own faces on one union vertex array -- against the project's
own per-mesh kernels, mesh by mesh, and the CPU oracle: the ragged draw and the ragged point-to-triangle scan reproduce the
shared-faces launches bit for bit on every mesh, and utils.ragged_point_to_surface / ragged_point_to_point give the mean of
the per-mesh losses with the float64 gradient.  Face counts sit on the kernels' internal limits (ragged_loss_helpers)."""
import numpy as np
import pytest
import torch

import oracle
from helpers import bits, fp64_surface_gradient, rows_close
from geometrics_amd import _lib, meshgen, ops, ragged, utils
from geometrics_amd.tri_distance import tri_distance_indexed
from ragged_loss_helpers import RaggedBatch, batch_a, batch_b
from test_ops_parity_gpu import ROW_FLOOR_ULPS, ROW_RTOL_SURFACE

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5        # the project's loss bar


def dev(a, gpu, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t.requires_grad_(True) if grad else t


class OnDevice:
    """A RaggedBatch on the device with its grouping (ragged.group_faces, checked against numpy in the host tests)."""

    def __init__(self, rb, gpu):
        self.rb, self.b = rb, rb.b
        self.verts, self.faces, self.face_mesh = dev(rb.verts, gpu), dev(rb.faces, gpu), dev(rb.face_mesh, gpu)
        self.face_list, self.face_off = ragged.group_faces(self.face_mesh, rb.b, self.faces)
        want_list, want_off = rb.grouping()
        assert np.array_equal(self.face_list.cpu().numpy(), want_list) and np.array_equal(self.face_off.cpu().numpy(), want_off)
        self.mesh = [tuple(dev(x, gpu) for x in rb.faces_of(m)) for m in range(rb.b)]      # (union ids, faces) per mesh

    def local(self, m, union_ids):
        """Positions inside mesh m of union face ids that belong to it."""
        ids = self.mesh[m][0]
        pos = torch.searchsorted(ids, union_ids)
        assert torch.equal(ids[pos.clamp(max=ids.numel() - 1)], union_ids), "a face of another mesh"
        return pos


@pytest.fixture(scope="module")
def batches(gpu):
    return {"a": OnDevice(batch_a(), gpu), "b": OnDevice(batch_b(), gpu)}


def _draw_ragged(d, num, uniforms=None, rng_state=None, points=True):
    dv = d.verts.device
    choices = torch.full((d.b, num), -1, dtype=torch.int64, device=dv)
    u, v = torch.zeros(d.b, num, device=dv), torch.zeros(d.b, num, device=dv)
    pts = torch.zeros(d.b, num, 3, device=dv) if points else None
    _lib.call("geom_draw_samples_ragged_f32", d.b, d.verts.shape[0], d.verts, d.faces.shape[0], d.faces, d.face_list, d.face_off, num,
              uniforms, rng_state, choices, u, v, pts)
    return choices, u, v, pts


def _scan_ragged(d, xyz, flags):
    n, dv = xyz.shape[1], xyz.device
    dist = torch.zeros(d.b, n, device=dv)
    point, index = torch.full((d.b, n), -1, dtype=torch.int32, device=dv), torch.full((d.b, n), -1, dtype=torch.int32, device=dv)
    _lib.call("geom_tri_distance_ragged_f32", d.b, n, xyz, d.verts.shape[0], d.verts, d.faces.shape[0], d.faces, d.face_list, d.face_off,
              dist, point, index, flags)
    return dist, point, index


# ------------------------------------------------------------------------------------------------ draws ----
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("num", [1, 1025])
def test_draws_from_uniforms_are_the_per_mesh_draws(gpu, batches, name, num):
    """Mesh m of the ragged launch against geom_draw_samples_f32 on (the union verts, the faces of mesh m) with mesh m's
    uniforms: the same position in the mesh's face list, u, v and points bit for bit."""
    d = batches[name]
    uniforms = torch.rand(3, d.b, num, device=gpu, generator=torch.Generator(device=gpu).manual_seed(3 + num))
    choices, u, v, pts = _draw_ragged(d, num, uniforms=uniforms)
    nv = d.verts.shape[0]
    for m, (ids, faces_m) in enumerate(d.mesh):
        c1 = torch.empty(1, num, dtype=torch.int64, device=gpu)
        u1, v1, p1 = torch.empty(1, num, device=gpu), torch.empty(1, num, device=gpu), torch.empty(1, num, 3, device=gpu)
        _lib.call("geom_draw_samples_f32", 1, nv, d.verts, faces_m.shape[0], faces_m, num, uniforms[:, m:m + 1].contiguous(), c1, u1, v1)
        _lib.call("geom_sample_faces_fwd_f32", 1, nv, d.verts, faces_m.shape[0], faces_m, num, c1, u1, v1, p1)
        assert torch.equal(choices[m], ids[c1[0]]), "mesh %d (%d faces)" % (m, ids.numel())
        assert torch.equal(u[m].view(torch.int32), u1[0].view(torch.int32)) and torch.equal(v[m].view(torch.int32), v1[0].view(torch.int32))
        assert torch.equal(pts[m].view(torch.int32), p1[0].view(torch.int32)), "mesh %d (%d faces)" % (m, ids.numel())


def test_draws_from_the_generator_are_the_batched_draws(gpu):
    """B copies of one topology, their faces interleaved in the union: the ragged launch against geom_draw_samples_rng_f32 at
    b = B from the same generator state, bit for bit; the stream position has advanced by one and the arrival counter is back
    at zero."""
    B, num = 3, 1025
    V, F = meshgen.icosphere(2)
    nv, nf = V.shape[0], F.shape[0]
    copies = meshgen.jittered_batch(V, B)
    union_faces = np.empty((nf * B, 3), np.int64)
    ids = np.empty(nf * B, np.int64)
    for m in range(B):                       # union face f * B + m = face f of mesh m: interleaved, each mesh in F's order
        union_faces[m::B] = F + m * nv
        ids[m::B] = m
    verts_b, faces = dev(copies, gpu), dev(F, gpu)
    verts_u, faces_u = dev(copies.reshape(-1, 3), gpu), dev(union_faces, gpu)
    face_list, face_off = ragged.group_faces(dev(ids, gpu), B, faces_u)
    seeded = ops.manual_seed(77, gpu, mesh_offset=5)
    state_b, state_r = seeded.clone(), seeded.clone()
    cb = torch.empty(B, num, dtype=torch.int64, device=gpu)
    ub, vb, pb = torch.empty(B, num, device=gpu), torch.empty(B, num, device=gpu), torch.empty(B, num, 3, device=gpu)
    _lib.call("geom_draw_samples_rng_f32", B, nv, verts_b, nf, faces, num, state_b, cb, ub, vb, pb)
    cr, ur, vr, pr = (torch.empty_like(t) for t in (cb, ub, vb, pb))
    _lib.call("geom_draw_samples_ragged_f32", B, B * nv, verts_u, B * nf, faces_u, face_list, face_off, num, None, state_r, cr, ur, vr, pr)
    assert torch.equal(cr, cb * B + torch.arange(B, device=gpu).view(B, 1))
    for got, want in ((ur, ub), (vr, vb), (pr, pb)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert state_r.tolist() == state_b.tolist() == [77, 1, 0, 5]


# ------------------------------------------------------------------------------------------------- scan ----
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("n_gt", [1, 65, 130])
def test_scan_is_the_per_mesh_scan(gpu, batches, name, n_gt):
    """dist / point bit-identical to tri_distance_indexed on every mesh alone, index mapped through the mesh's face list;
    culled == brute force, with and without FIX_REGION6; both equal the CPU oracle per mesh."""
    d = batches[name]
    xyz_np = meshgen.gt_cloud(d.b, n_gt, first=3)
    xyz = dev(xyz_np, gpu)
    for fix6 in (0, _lib.FLAG_FIX_REGION6):
        culled = _scan_ragged(d, xyz, fix6)
        brute = _scan_ragged(d, xyz, fix6 | _lib.FLAG_TRI_BRUTE_FORCE)
        for got, want in zip(culled, brute):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "culled != brute force (flags %d)" % fix6
        dist, point, index = (t.cpu().numpy() for t in culled)
        for m, (ids, faces_m) in enumerate(d.mesh):
            what = "mesh %d (%d faces), flags %d" % (m, ids.numel(), fix6)
            d1, p1, i1 = tri_distance_indexed(xyz[m:m + 1], d.verts[None], faces_m, flags=fix6, use_workspace=False)
            assert np.array_equal(bits(dist[m]), bits(d1[0].cpu().numpy())), what
            assert np.array_equal(point[m], p1[0].cpu().numpy()), what
            assert np.array_equal(index[m], ids.cpu().numpy()[i1[0].cpu().numpy()]), what
            od, op, oi = oracle.tri_scan_indexed(xyz_np[m:m + 1], d.rb.verts[None], d.rb.faces_of(m)[1], fix6)
            assert np.array_equal(bits(dist[m]), bits(od[0])) and np.array_equal(point[m], op[0]), what + " (oracle)"
            assert np.array_equal(index[m], d.rb.faces_of(m)[0][oi[0]]), what + " (oracle)"


# -------------------------------------------------------------------------------------------- fail-safe ----
def test_a_mesh_without_faces_and_one_with_too_many_fail_safe(gpu, batches):
    """The two entry points alone (nothing dereferences their outputs).  Mesh id 2 of five owns no face: every choice is a
    valid face id, its u / v / points are NaN, its scan row is (NaN, 0, 0), and the other meshes' rows are those of the batch
    without the empty mesh.  A mesh of 16385 faces (more than the draw's table holds): its first listed face, NaN."""
    full, num, n_gt = batches["b"], 65, 65
    rb = batch_b()
    rb.face_mesh = rb.face_mesh + (rb.face_mesh >= 2)              # ids 0, 1, 3, 4
    rb.b, rb.sizes = 5, rb.sizes[:2] + (0,) + rb.sizes[2:]
    d = OnDevice(rb, gpu)
    keep = [0, 1, 3, 4]
    nft = d.faces.shape[0]
    u4 = torch.rand(3, 4, num, device=gpu, generator=torch.Generator(device=gpu).manual_seed(9))
    u5 = torch.zeros(3, 5, num, device=gpu)
    u5[:, keep] = u4
    want = _draw_ragged(full, num, uniforms=u4)
    got = _draw_ragged(d, num, uniforms=u5)
    assert int(got[0].min()) >= 0 and int(got[0].max()) < nft
    assert bool(torch.isnan(got[1][2]).all()) and bool(torch.isnan(got[2][2]).all()) and bool(torch.isnan(got[3][2]).all())
    for g, w in zip(got, want):
        assert torch.equal(g[keep].reshape(4, -1).view(torch.int32 if g.dtype == torch.float32 else g.dtype),
                           w.reshape(4, -1).view(torch.int32 if w.dtype == torch.float32 else w.dtype))
    state = ops.manual_seed(5, gpu).clone()
    rng = _draw_ragged(d, num, rng_state=state)                    # the empty mesh's workgroup reports in all the same
    assert state.tolist() == [5, 1, 0, 0] and int(rng[0].min()) >= 0 and int(rng[0].max()) < nft
    assert bool(torch.isnan(rng[1][2]).all()) and bool(torch.isfinite(rng[1][keep]).all())
    xyz4 = dev(meshgen.gt_cloud(4, n_gt, first=8), gpu)
    xyz5 = torch.zeros(5, n_gt, 3, device=gpu)
    xyz5[keep] = xyz4
    for flags in (0, _lib.FLAG_TRI_BRUTE_FORCE):
        want = _scan_ragged(full, xyz4, flags)
        dist, point, index = _scan_ragged(d, xyz5, flags)
        assert bool(torch.isnan(dist[2]).all()) and not bool(point[2].any()) and not bool(index[2].any())
        assert torch.equal(dist[keep].view(torch.int32), want[0].view(torch.int32))
        assert torch.equal(point[keep], want[1]) and torch.equal(index[keep], want[2])
    # more faces than the table holds: 16385 copies of one triangle as mesh 0, three faces of an icosahedron as mesh 1
    big = RaggedBatch((20, 3), 2)
    first = big.faces_of(0)[1][:1]
    big.faces = np.concatenate((np.repeat(first, 16385, 0), big.faces_of(1)[1]))
    big.face_mesh = np.concatenate((np.zeros(16385, np.int64), np.ones(3, np.int64)))
    big.sizes = (16385, 3)
    dbig = OnDevice(big, gpu)
    c, u, v, p = _draw_ragged(dbig, num, uniforms=u4[:, :2].contiguous())
    assert bool((c[0] == 0).all()) and bool(torch.isnan(u[0]).all()) and bool(torch.isnan(v[0]).all()) and bool(torch.isnan(p[0]).all())
    assert int(c[1].min()) >= 16385 and int(c[1].max()) < 16388 and bool(torch.isfinite(p[1]).all())


# ------------------------------------------------------------------------------------------------- loss ----
def _loop(fn, d, gt, draws, num, f1=False):
    """The baseline: one per-mesh call of the batched loss per mesh, on the union verts and the mesh's own faces."""
    choices, u, v = draws
    verts = d.verts.detach().clone().requires_grad_(True)
    losses, sq = [], []
    ops.scan_capture = {} if f1 else None
    try:
        for m, (ids, faces_m) in enumerate(d.mesh):
            dr = (d.local(m, choices[m])[None], u[m:m + 1], v[m:m + 1])
            losses.append(fn(verts[None], {"faces": faces_m}, gt[m:m + 1], num=num, draws=dr))
            if f1:
                sq.append((ops.scan_capture["sq_gt"].clone(), ops.scan_capture["sq_pred"].clone()))
    finally:
        ops.scan_capture = None
    return losses, sq


def _replayed_draws(d, num, gpu):
    return ops.draw_samples_ragged(d.verts, d.faces, d.face_list, d.face_off, num, generator=torch.Generator(device=gpu).manual_seed(21 + num))


def _fp64_union_gradient(d, gt, draws, two_sided):
    """helpers.fp64_surface_gradient per mesh (its own faces on the union verts, b = 1), scatter-added into the union and
    averaged over the meshes: (loss, grad, mass, floor)."""
    choices, u, v = (t.cpu() for t in draws)
    total, parts = 0.0, [np.zeros(d.rb.verts.shape, np.float64) for _ in range(3)]
    for m in range(d.b):
        ids, faces_m = d.rb.faces_of(m)
        local = np.searchsorted(ids, choices[m].numpy())
        loss, *gmf = fp64_surface_gradient(d.rb.verts[None], faces_m, gt[m:m + 1].cpu().numpy(), local[None], u[m:m + 1].numpy(),
                                           v[m:m + 1].numpy(), two_sided)
        total += loss / d.b
        for acc, x in zip(parts, gmf):
            acc += x[0] / d.b
    return (total,) + tuple(parts)


@pytest.mark.parametrize("fn_name, two_sided", [("point_to_surface", False), ("point_to_point", True)])
@pytest.mark.parametrize("name, n_gt, num", [("a", 130, 1025), ("a", 65, 1), ("b", 1, 1025)])
def test_loss_with_replayed_draws_is_the_mean_of_the_loop_and_its_gradient_float64s(gpu, batches, fn_name, two_sided, name, n_gt, num):
    """|L - mean of the loop's losses| <= 1e-5 of that mean; the gradient element by element against float64 at the surface
    loss's row bound, under an upstream gradient other than 1."""
    d = batches[name]
    gt = dev(meshgen.gt_cloud(d.b, n_gt, first=5), gpu)
    draws = _replayed_draws(d, num, gpu)
    losses, _ = _loop(getattr(utils, "batch_" + fn_name), d, gt, draws, num)
    want = float(torch.stack(losses).detach().double().mean())
    verts = d.verts.detach().clone().requires_grad_(True)
    loss = getattr(utils, "ragged_" + fn_name)(verts, d.faces, d.face_mesh, gt, num=num, draws=draws)
    upstream = 0.37
    (loss * upstream).backward()
    print("%s %s n_gt %d num %d: loss %.9g, loop mean %.9g, rel %.3g" % (fn_name, name, n_gt, num, float(loss), want,
                                                                       abs(float(loss) - want) / abs(want)))
    assert abs(float(loss) - want) <= LOSS_RTOL * abs(want)
    exact_loss, grad, mass, floor = _fp64_union_gradient(d, gt, draws, two_sided)
    assert abs(float(loss) - exact_loss) <= LOSS_RTOL * abs(exact_loss)
    worst = rows_close(verts.grad.cpu().numpy(), upstream * grad, upstream * mass, ROW_RTOL_SURFACE, "ragged " + fn_name,
                       floor=upstream * floor, floor_ulps=ROW_FLOOR_ULPS)
    print("    worst gradient element at %.3g of its bound" % worst)
    assert verts.grad.shape == verts.shape and bool((verts.grad != 0).any())


@pytest.mark.parametrize("fn_name", ["point_to_surface", "point_to_point"])
def test_f1_is_the_f_score_of_the_loops_distances(gpu, batches, fn_name):
    d, n_gt, num = batches["a"], 130, 1025
    draws = _replayed_draws(d, num, gpu)
    # gt close to the meshes, so that distances fall on both sides of the threshold: sampled points of each mesh, moved a little
    near = ops.draw_samples_ragged(d.verts, d.faces, d.face_list, d.face_off, n_gt, generator=torch.Generator(device=gpu).manual_seed(2),
                                   with_points=True)[3]
    gt = (near + dev(meshgen.gt_cloud(d.b, n_gt, first=5), gpu) * 0.02).contiguous()
    _, sq = _loop(getattr(utils, "batch_" + fn_name), d, gt, draws, num, f1=True)
    want = utils._f_score(torch.cat([a for a, _ in sq]), torch.cat([b for _, b in sq]), num)
    loss, f1 = getattr(utils, "ragged_" + fn_name)(d.verts, d.faces, d.face_mesh, gt, num=num, f1=True, draws=draws)
    print("%s: F1 %.6g (loop %.6g)" % (fn_name, f1, want))
    assert isinstance(f1, float) and f1 == want and 0.0 < want < 1.0 and bool(torch.isfinite(loss))


def test_one_captured_call_draws_fresh_samples_on_every_replay(gpu, batches):
    """No host read and no host-side generator bookkeeping: a captured call (forward and backward) replays, the stream position
    advances on the device, every replay draws other samples and the loss stays finite."""
    d, num = batches["b"], 130
    gt = dev(meshgen.gt_cloud(d.b, 65, first=5), gpu)
    verts = d.verts.detach().clone().requires_grad_(True)
    state = ops.manual_seed(31, gpu)
    for _ in range(2):
        utils.ragged_point_to_surface(verts, d.faces, d.face_mesh, gt, num=num).backward()
    torch.cuda.synchronize()
    assert state.tolist()[1] == 2
    verts.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = utils.ragged_point_to_surface(verts, d.faces, d.face_mesh, gt, num=num)
        loss.backward()
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append((float(loss), verts.grad.clone()))
    assert state.tolist()[1:3] == [4, 0]
    assert all(np.isfinite(l) for l, _ in seen) and seen[0][0] != seen[1][0] and not torch.equal(seen[0][1], seen[1][1])
    assert all(bool(torch.isfinite(g).all()) for _, g in seen)
