"""-m gpu: the ORDERED backward of the ragged surface loss (geom_surface_finalize_ragged_f32 + geom_surface_gather_ragged_f32)
and its per-mesh weights.  Mesh by mesh the gradient carries the bits of the batched finalize + gather pair on that mesh alone;
it holds the float64 row bound of the surface loss, agrees with the scatter route, repeats bit for bit, fails safe (a mesh
without faces, a mesh with more faces than the finalize launch's LDS holds, a face that joins two meshes) and is one launch.
Batches and bounds are those of tests/test_ragged_loss_gpu.py."""
import numpy as np
import pytest
import torch

from helpers import fp64_surface_gradient, rows_close
from geometrics_amd import _lib, meshgen, ops, utils
from ragged_loss_helpers import RaggedBatch, batch_a, batch_b
from test_ops_parity_gpu import ROW_FLOOR_ULPS, ROW_RTOL_SURFACE
from test_ragged_loss_gpu import LOSS_RTOL, OnDevice, _loop, _replayed_draws, dev

pytestmark = pytest.mark.gpu

LOSSES = [("point_to_surface", False), ("point_to_point", True)]
CASES = [("a", 130, 1025), ("a", 65, 1), ("b", 1, 1025), ("b", 130, 8100)]      # the last: num + n_gt > 8192, the scratch variant
UPSTREAM = 0.37
# a zero, a negative, non-powers of two; little cancellation in sum_m w[m] L_m (the loss bar is relative to that sum)
WEIGHTS = (0.0, -0.25, 0.3, 1.0, 2.7, 0.6, 1.3, 0.9)


@pytest.fixture(scope="module")
def batches(gpu):
    return {"a": OnDevice(batch_a(), gpu), "b": OnDevice(batch_b(), gpu)}


def _weights(d, gpu):
    return torch.tensor(WEIGHTS[:d.b], dtype=torch.float32, device=gpu)


def _run(d, fn_name, gt, draws, num, weight=1.0, capture=False):
    """One eager forward + backward under the upstream gradient -> (loss, grad [Vt,3], what the forward left on the device)."""
    verts = d.verts.detach().clone().requires_grad_(True)
    ops.scan_capture = {} if capture else None
    try:
        loss = getattr(utils, "ragged_" + fn_name)(verts, d.faces, d.face_mesh, gt, num=num, draws=draws, weight=weight)
        seen = ops.scan_capture
    finally:
        ops.scan_capture = None
    (grad,) = torch.autograd.grad(loss, verts, torch.tensor(UPSTREAM, device=gt.device))
    return loss.detach(), grad, seen


def _per_mesh_pair(d, m, seen, gt, two_sided, weight):
    """geom_surface_finalize_w_f32 + geom_surface_gather_w_f32 at b = 1 on the union verts with the faces of mesh m in ascending
    union id, fed what the ragged forward left on the device, the ragged call's coefficients and w[m:m+1] -> grad [Vt,3]."""
    ids, faces_m = d.mesh[m]
    gpu, nv, nf = gt.device, d.verts.shape[0], faces_m.shape[0]
    num, n_gt = seen["choices"].shape[1], gt.shape[1]
    row = lambda t: t[m:m + 1].contiguous()
    choices = d.local(m, seen["choices"][m])[None].contiguous()
    if two_sided:
        idx_p, index, closest, weights, sq_other = row(seen["idx_gt"]), None, None, None, row(seen["sq_gt"])
    else:
        index = d.local(m, seen["tri_index"][m].long()).to(torch.int32)[None].contiguous()
        idx_p, closest, weights, sq_other = None, row(seen["closest"]), row(seen["weights"]), row(seen["sq"])
    order = torch.empty(_lib.lib().geom_surface_order_words(1, nf, num, n_gt), dtype=torch.int32, device=gpu)
    loss, out = torch.empty((), device=gpu), torch.empty(1, nv, 3, device=gpu)
    wm = None if weight is None else weight[m:m + 1]
    _lib.call("geom_surface_finalize_w_f32", 1, nf, num, choices, row(seen["u"]), row(seen["v"]), row(seen["points"]), n_gt, row(gt),
              row(seen["idx_pred"]), idx_p, index, closest, weights, row(seen["sq_pred"]), sq_other, 1.0, 1.0,
              utils.LOSS_SCALE / (d.b * num), utils.LOSS_SCALE / (d.b * n_gt), 1, 0, order, loss, wm)
    vf_ptr, vf_item = ops.vertex_faces(faces_m, nv)
    _lib.call("geom_surface_gather_w_f32", 1, nv, nf, vf_ptr, vf_item, num, n_gt, 1, order, torch.tensor(UPSTREAM, device=gpu), wm, out)
    return out[0]


def _rows(d, m):
    return slice(d.rb.vert_off[m], d.rb.vert_off[m + 1])


_shared = {}


def _case(gpu, batches, name, n_gt, num, two_sided):
    """Inputs and the float64 reference of a case, made once: gt, draws, and PER MESH (loss, grad, mass, floor) of
    helpers.fp64_surface_gradient on the mesh's own faces over the union verts at b = 1."""
    key = (name, n_gt, num, two_sided)
    if key not in _shared:
        d = batches[name]
        gt = dev(meshgen.gt_cloud(d.b, n_gt, first=5), gpu)
        draws = _replayed_draws(d, num, gpu)
        choices, u, v = (t.cpu() for t in draws)
        parts = []
        for m in range(d.b):
            ids, faces_m = d.rb.faces_of(m)
            local = np.searchsorted(ids, choices[m].numpy())
            parts.append(fp64_surface_gradient(d.rb.verts[None], faces_m, gt[m:m + 1].cpu().numpy(), local[None], u[m:m + 1].numpy(),
                                               v[m:m + 1].numpy(), two_sided))
        _shared[key] = (gt, draws, parts)
    return _shared[key]


def _fp64(parts, w):
    """(1/B) sum_m w[m] * (mesh m's float64 loss and gradient); mass and floor with |w[m]|."""
    b = len(parts)
    loss = sum(wm * p[0] for wm, p in zip(w, parts)) / b
    grad = sum(wm * p[1][0] for wm, p in zip(w, parts)) / b
    mass = sum(abs(wm) * p[2][0] for wm, p in zip(w, parts)) / b
    floor = sum(abs(wm) * p[3][0] for wm, p in zip(w, parts)) / b
    return loss, grad, mass, floor


# ---------------------------------------------------------------------------------- (a) the bit contract ----
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fn_name, two_sided", LOSSES)
@pytest.mark.parametrize("name, n_gt, num", CASES)
def test_every_mesh_carries_the_bits_of_the_batched_pair_on_that_mesh_alone(gpu, batches, fn_name, two_sided, name, n_gt, num, weighted):
    d = batches[name]
    gt, draws, _ = _case(gpu, batches, name, n_gt, num, two_sided)
    w = _weights(d, gpu) if weighted else None
    _, grad, seen = _run(d, fn_name, gt, draws, num, weight=1.0 if w is None else w, capture=True)
    assert grad.shape == d.verts.shape and bool((grad != 0).any()) and bool(torch.isfinite(grad).all())
    for m in range(d.b):
        want = _per_mesh_pair(d, m, seen, gt, two_sided, w)
        assert torch.equal(grad[_rows(d, m)], want[_rows(d, m)]), "mesh %d (%d faces)" % (m, d.rb.sizes[m])
        assert bool((want[_rows(d, m)] != 0).any()) or (weighted and WEIGHTS[m] == 0.0)


# ------------------------------------------------------------------------------------------ (b) float64 ----
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fn_name, two_sided", LOSSES)
@pytest.mark.parametrize("name, n_gt, num", CASES)
def test_gradient_holds_the_float64_row_bound_and_the_loss_is_the_weighted_mean(gpu, batches, fn_name, two_sided, name, n_gt, num, weighted):
    d = batches[name]
    gt, draws, parts = _case(gpu, batches, name, n_gt, num, two_sided)
    w = WEIGHTS[:d.b] if weighted else (1.0,) * d.b
    loss, grad, _ = _run(d, fn_name, gt, draws, num, weight=_weights(d, gpu) if weighted else 1.0)
    exact_loss, exact, mass, floor = _fp64(parts, w)
    losses, _ = _loop(getattr(utils, "batch_" + fn_name), d, gt, draws, num)
    want = sum(wm * float(l.detach().double()) for wm, l in zip(w, losses)) / d.b
    print("%s %s n_gt %d num %d weighted %d: loss %.9g, loop %.9g (rel %.3g), float64 %.9g" % (
        fn_name, name, n_gt, num, weighted, float(loss), want, abs(float(loss) - want) / abs(want), exact_loss))
    assert abs(float(loss) - want) <= LOSS_RTOL * abs(want)
    assert abs(float(loss) - exact_loss) <= LOSS_RTOL * abs(exact_loss)
    worst = rows_close(grad.cpu().numpy(), UPSTREAM * exact, UPSTREAM * mass, ROW_RTOL_SURFACE, "ragged ordered " + fn_name,
                       floor=UPSTREAM * floor, floor_ulps=ROW_FLOOR_ULPS)
    print("    worst gradient element at %.3g of its bound" % worst)


# ------------------------------------------------------------------------- (c) against the scatter route ----
@pytest.mark.parametrize("fn_name, two_sided", LOSSES)
@pytest.mark.parametrize("name, n_gt, num", CASES)
def test_the_scatter_route_gives_the_same_loss_bits_and_the_same_gradient_within_the_bound(gpu, batches, monkeypatch, fn_name, two_sided,
                                                                                           name, n_gt, num):
    d = batches[name]
    gt, draws, parts = _case(gpu, batches, name, n_gt, num, two_sided)
    loss, grad, _ = _run(d, fn_name, gt, draws, num)
    monkeypatch.setattr(ops, "ragged_backward", "scatter")
    loss_s, grad_s, _ = _run(d, fn_name, gt, draws, num)
    assert torch.equal(loss.view(torch.int32), loss_s.view(torch.int32))
    _, _, mass, floor = _fp64(parts, (1.0,) * d.b)
    worst = rows_close(grad.cpu().numpy(), grad_s.double().cpu().numpy(), UPSTREAM * mass, ROW_RTOL_SURFACE, "ordered vs scatter " + fn_name,
                       floor=UPSTREAM * floor, floor_ulps=ROW_FLOOR_ULPS)
    print("%s %s n_gt %d num %d: ordered against scatter, worst element at %.3g of the bound" % (fn_name, name, n_gt, num, worst))
    with pytest.raises(RuntimeError, match="per-mesh weights"):     # the scatter kernels know no mesh
        _run(d, fn_name, gt, draws, num, weight=_weights(d, gpu))


# ------------------------------------------------------------------------------------ (d) repeatability ----
@pytest.mark.parametrize("fn_name, two_sided", LOSSES)
@pytest.mark.parametrize("name, n_gt, num", CASES)
def test_five_passes_give_the_same_bits(gpu, batches, fn_name, two_sided, name, n_gt, num):
    d = batches[name]
    gt, draws, _ = _case(gpu, batches, name, n_gt, num, two_sided)
    w = _weights(d, gpu)
    first = _run(d, fn_name, gt, draws, num, weight=w)
    for _ in range(4):
        again = _run(d, fn_name, gt, draws, num, weight=w)
        assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1], again[1])


# ---------------------------------------------------------------------------------------- (e) fail-safe ----
@pytest.mark.parametrize("fn_name, two_sided", LOSSES)
def test_a_mesh_without_faces_leaves_the_other_meshes_their_bits(gpu, batches, fn_name, two_sided):
    """Mesh id 2 of five owns no face.  Its points are binned nowhere; the other meshes' rows are those of the four-mesh batch
    (the five-mesh call with weight 5/4: both coefficients are then the correctly rounded 750 / n)."""
    full, num, n_gt = batches["b"], 130, 65
    rb = batch_b()
    rb.face_mesh = rb.face_mesh + (rb.face_mesh >= 2)              # ids 0, 1, 3, 4
    rb.b, rb.sizes = 5, rb.sizes[:2] + (0,) + rb.sizes[2:]
    d, keep = OnDevice(rb, gpu), [0, 1, 3, 4]
    gt4 = dev(meshgen.gt_cloud(4, n_gt, first=5), gpu)
    gt5 = torch.zeros(5, n_gt, 3, device=gpu)
    gt5[keep] = gt4
    draws4 = _replayed_draws(full, num, gpu)
    draws5 = []
    for t in draws4:                                               # the empty mesh's samples: face 0 (another mesh's), u = v = 0.5
        t5 = torch.full((5, num), 0.5, device=gpu).to(t.dtype) if t.dtype == torch.float32 else torch.zeros(5, num, dtype=t.dtype, device=gpu)
        t5[keep] = t
        draws5.append(t5)
    _, want, _ = _run(full, fn_name, gt4, draws4, num)
    _, got, _ = _run(d, fn_name, gt5, tuple(draws5), num, weight=1.25)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def _per_mesh_reference(d, m, fn_name, two_sided, gt, draws, num):
    _, grad, seen = _run(d, fn_name, gt, draws, num, capture=True)
    return grad, _per_mesh_pair(d, m, seen, gt, two_sided, None)


@pytest.mark.parametrize("fn_name, two_sided", LOSSES)
def test_a_mesh_with_more_faces_than_the_launch_holds_gets_nan_and_the_other_its_bits(gpu, fn_name, two_sided):
    """One triangle repeated until mesh 0 has one face more than the finalize launch's LDS holds beside num + n_gt points (the
    cap the entry point reports); mesh 1: three faces.  Mesh 0's workgroup orders nothing (its faces get a negative count):
    its three vertices are NaN, mesh 1's rows are those of the batched pair on mesh 1 alone, every other vertex is 0."""
    num, n_gt = 8, 8
    cap = _lib.lib().geom_surface_ragged_face_cap(1 << 30, num, n_gt)
    assert 16384 < cap < 40000
    big = RaggedBatch((20, 3), 2)
    first = big.faces_of(0)[1][:1]
    big.faces = np.concatenate((np.repeat(first, cap + 1, 0), big.faces_of(1)[1]))
    big.face_mesh = np.concatenate((np.zeros(cap + 1, np.int64), np.ones(3, np.int64)))
    big.sizes = (cap + 1, 3)
    d = OnDevice(big, gpu)
    g = torch.Generator(device=gpu).manual_seed(4)
    choices = torch.stack((torch.randint(0, cap + 1, (num,), device=gpu, generator=g),
                           torch.randint(cap + 1, cap + 4, (num,), device=gpu, generator=g)))
    u, v = torch.rand(2, num, device=gpu, generator=g).sqrt(), torch.rand(2, num, device=gpu, generator=g)
    gt = dev(meshgen.gt_cloud(2, n_gt, first=5), gpu)
    grad, want = _per_mesh_reference(d, 1, fn_name, two_sided, gt, (choices, u, v), num)
    own = torch.zeros(d.verts.shape[0], dtype=torch.bool, device=gpu)
    own[torch.from_numpy(first.reshape(-1)).to(gpu)] = True
    assert bool(torch.isnan(grad[own]).all())
    assert torch.equal(grad[_rows(d, 1)], want[_rows(d, 1)]) and bool((grad[_rows(d, 1)] != 0).any())
    rest = ~own
    rest[_rows(d, 1)] = False
    assert not bool(grad[rest].any())


@pytest.mark.parametrize("fn_name, two_sided", LOSSES)
def test_with_weights_a_face_that_joins_two_meshes_gives_nan_at_the_shared_vertices_only(gpu, fn_name, two_sided):
    rb, num, n_gt = batch_b(), 130, 65
    shared = int(rb.faces_of(1)[1][0, 0])                           # a vertex of mesh 1 that its faces use ...
    rb.faces[rb.faces_of(0)[0][0], 2] = shared                      # ... becomes a corner of a face of mesh 0
    d = OnDevice(rb, gpu)
    gt = dev(meshgen.gt_cloud(d.b, n_gt, first=5), gpu)
    draws = _replayed_draws(d, num, gpu)
    _, plain, _ = _run(d, fn_name, gt, draws, num)
    assert bool(torch.isfinite(plain).all())                        # without weights: the plain sum, as the scatter gives
    _, grad, _ = _run(d, fn_name, gt, draws, num, weight=_weights(d, gpu))
    bad = torch.isnan(grad).any(1)
    assert bad.nonzero().flatten().tolist() == [shared] and bool(torch.isnan(grad[shared]).all())


# ------------------------------------------------------------------------------------ (f) graph capture ----
@pytest.mark.parametrize("fn_name", ["point_to_surface", "point_to_point"])
def test_a_captured_forward_and_backward_replays_the_eager_bits_on_fresh_draws(gpu, batches, fn_name):
    d, num = batches["b"], 130
    gt = dev(meshgen.gt_cloud(d.b, 65, first=5), gpu)
    w = _weights(d, gpu) + 0.5
    fn = getattr(utils, "ragged_" + fn_name)
    verts = d.verts.detach().clone().requires_grad_(True)
    state = ops.manual_seed(47, gpu)
    eager = []

    def eager_step():      # nothing of its autograd graph outlives the call: an accumulator of verts.grad made here, on the
        verts.grad = None  # ambient stream, must not be met again by the captured backward (a second stream in the graph)
        loss = fn(verts, d.faces, d.face_mesh, gt, num=num, weight=w)
        loss.backward()
        eager.append((loss.detach().clone(), verts.grad.clone()))

    for _ in range(4):                                              # stream positions 0 .. 3
        eager_step()
    torch.cuda.synchronize()
    assert state.tolist()[1] == 4 and not torch.equal(eager[2][1], eager[3][1])
    state.copy_(torch.tensor([47, 2, 0, 0], dtype=torch.int64))     # back to position 2, in place: the graph keeps the address
    verts.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = fn(verts, d.faces, d.face_mesh, gt, num=num, weight=w)
        loss.backward()
    for want_loss, want_grad in eager[2:]:
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach().view(torch.int32), want_loss.view(torch.int32)) and torch.equal(verts.grad, want_grad)
    assert state.tolist()[1:3] == [4, 0]


# ------------------------------------------------------------------------------------- (g) launch count ----
@pytest.mark.parametrize("fn_name", ["point_to_surface", "point_to_point"])
def test_the_backward_is_one_launch(gpu, batches, monkeypatch, fn_name):
    d, num = batches["b"], 130
    gt = dev(meshgen.gt_cloud(d.b, 65, first=5), gpu)
    verts = d.verts.detach().clone().requires_grad_(True)
    loss = getattr(utils, "ragged_" + fn_name)(verts, d.faces, d.face_mesh, gt, num=num, draws=_replayed_draws(d, num, gpu),
                                               weight=_weights(d, gpu))
    names, call = [], _lib.call

    def recording_call(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(ops._lib, "call", recording_call)
    loss.backward()
    monkeypatch.setattr(ops._lib, "call", call)
    assert names == ["geom_surface_gather_ragged_f32"]              # no zero-fill, no scatter entry point, no table built here
