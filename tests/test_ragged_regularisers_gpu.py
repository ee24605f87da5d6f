"""GPU: utils.ragged_stage_regularisers / ragged_calc_edge (ops.RaggedStageRegularisers, csrc/regularizers.hip) on union meshes
whose meshes interleave -- value and every element of both gradients and of the saved Laplacian against float64 inside the
project's per-element bounds, equal to the per-mesh loop, stacking with per-mesh weights, bit reproducibility, the fail-safes,
graph capture (no host read) -- and ragged.csr_from_faces against the dense route."""
import numpy as np
import pytest
import torch

from geometrics_amd import layers, meshgen, ops, ragged, utils
from oracle import ref_ops
from ragged_reg_helpers import BATCHES, SCALAR_WEIGHTS, bounds, reference_value, union_chain
from test_ops_parity_gpu import ROW_FLOOR_ULPS, stage_regulariser_outputs_close
from helpers import rows_close

pytestmark = pytest.mark.gpu
GOUT = 0.7


def per_mesh_weights(b):
    """[b] weights that differ per mesh and include a 0 in every row."""
    return ([300.0 * (m + 1) for m in range(b - 1)] + [0.0], [0.0] + [20.0 + 5.0 * m for m in range(b - 1)],
            [300.0 if m != b // 2 else 0.0 for m in range(b)])


@pytest.fixture(scope="module")
def batches():
    return {name: make() for name, make in BATCHES.items()}


@pytest.fixture(scope="module")
def exacts(batches):
    """(exact, mass, floor, rtol) per (batch, weights kind): computed once, shared, left unchanged."""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            rb = batches[name]
            cache[name, kind] = bounds(rb, per_mesh_weights(rb.b) if kind == "per-mesh" else SCALAR_WEIGHTS, GOUT)
        return cache[name, kind]
    return get


class OnDevice:
    """A RegBatch's tensors on the GPU (fresh leaves for prev and cur) and the union's CSR from ALL faces."""

    def __init__(self, rb, gpu):
        self.prev, self.cur = rb.prev.to(gpu).requires_grad_(True), rb.cur.to(gpu).requires_grad_(True)
        self.faces, self.face_mesh, self.vert_mesh = rb.faces.to(gpu), rb.face_mesh.to(gpu), rb.vert_mesh.to(gpu)
        self.csr = ragged.csr_from_faces(rb.adj_faces.to(gpu), rb.vt)
        self.b = rb.b

    def loss(self, weights, **kw):
        a = dict(prev=self.prev, cur=self.cur, faces=self.faces, face_mesh=self.face_mesh, vert_mesh=self.vert_mesh, csr=self.csr, b=self.b)
        a.update(kw)
        return utils.ragged_stage_regularisers(a["prev"], a["cur"], a["faces"], a["face_mesh"], a["vert_mesh"], a["csr"], a["b"],
                                               lap_weight=weights[0], move_weight=weights[1], edge_weight=weights[2])


def on_device(weights, gpu):
    return tuple(torch.tensor(w, dtype=torch.float32, device=gpu) if isinstance(w, list) else w for w in weights)


def outputs(d, loss):
    """Backward of GOUT * loss -> {"lapd", "grad_cur", "grad_prev"} as numpy."""
    lapd = loss.grad_fn.saved_tensors[9]
    d.prev.grad = d.cur.grad = None
    (loss * GOUT).backward()
    return {"lapd": lapd.cpu().numpy(), "grad_cur": d.cur.grad.cpu().numpy(), "grad_prev": d.prev.grad.cpu().numpy()}


@pytest.mark.parametrize("kind", ["scalar", "per-mesh"])
@pytest.mark.parametrize("name", ["mixed", "edge-cut", "single"])
def test_value_and_every_element_against_float64(gpu, batches, exacts, name, kind):
    """The value within 1e-6 and every element of grad_cur, grad_prev and the saved lap(prev - cur) within (row_terms + 8) * 2^-24
    of its own term mass + one coordinate ulp per term (the bounds of ops.StageRegularisers), with scalar weights (300, 20, 300)
    and with [b] weights that differ per mesh and include a 0.  On "mixed" a kernel that ignores the ids is first shown to be
    far outside the value's bar.  One mesh: ops.StageRegularisers at b = 1 on the same data lies in the same bounds."""
    rb = batches[name]
    if name == "single" and kind == "per-mesh":
        kind = "scalar"
        weights = [[w] for w in SCALAR_WEIGHTS]                  # [1] tensors of the scalar weights: the same bounds
    else:
        weights = per_mesh_weights(rb.b) if kind == "per-mesh" else SCALAR_WEIGHTS
    exact, mass, floor, rtol = exacts(name, kind)
    want = float(exact["value"])
    if name == "mixed":
        assert (8 * rb.vt) % 256 != 0
        ignoring = float(reference_value(rb, weights, union_counts=True)[0].detach())
        assert abs(ignoring - want) > 1e-3 * abs(want), (ignoring, want)
    if name == "edge-cut":
        assert rb.ft > 8 * rb.vt
    d = OnDevice(rb, gpu)
    loss = d.loss(on_device(weights, gpu))
    got = outputs(d, loss)
    print("%s %s: value %.9g, float64 %.9g, relative error %.3g" % (name, kind, loss.item(), want, abs(loss.item() - want) / abs(want)))
    assert abs(loss.item() - want) <= 1e-6 * abs(want), (loss.item(), want)
    stage_regulariser_outputs_close(got, exact, mass, floor, rtol, "ragged %s %s" % (name, kind))
    if name == "single":
        p, c = rb.prev.to(gpu)[None].requires_grad_(True), rb.cur.to(gpu)[None].requires_grad_(True)
        csr = layers.adjacency_csr(rb.adj[0].to(gpu))
        faces = rb.local_faces[0].to(gpu)
        dense = ops.StageRegularisers.apply(p[:, rb.vids[0].to(gpu)], c[:, rb.vids[0].to(gpu)], faces, csr.rowptr, csr.col, csr.inv_deg,
                                            *SCALAR_WEIGHTS)
        (dense * GOUT).backward()
        assert abs(dense.item() - want) <= 1e-6 * abs(want)
        stage_regulariser_outputs_close({"grad_cur": c.grad[0].cpu().numpy(), "grad_prev": p.grad[0].cpu().numpy()}, exact, mass, floor, rtol,
                                        "ops.StageRegularisers at b = 1")


@pytest.mark.parametrize("name", ["mixed", "edge-cut"])
def test_equal_to_the_loop_over_the_meshes(gpu, batches, name):
    """The value is the mean of utils.stage_regularisers on every mesh alone (existing code: what tools/time_ragged_regularisers.py
    times against) at 1e-5."""
    rb = batches[name]
    d = OnDevice(rb, gpu)
    loss = d.loss(SCALAR_WEIGHTS)
    total = 0.0
    for m in range(rb.b):
        vids = rb.vids[m].to(gpu)
        info = {"adj_orig": rb.adj[m].to(gpu), "faces": rb.local_faces[m].to(gpu)}
        total += utils.stage_regularisers(d.prev.detach()[vids][None], d.cur.detach()[vids][None], info, lap_weight=SCALAR_WEIGHTS[0],
                                          move_weight=SCALAR_WEIGHTS[1], edge_weight=SCALAR_WEIGHTS[2]).item()
    assert abs(loss.item() - total / rb.b) <= 1e-5 * abs(total / rb.b), (loss.item(), total / rb.b)


def test_two_stages_stacked_with_per_mesh_weights_are_one_call(gpu, batches):
    """Two copies of "mixed" (other positions, other weights: two stages) as one union of 2b meshes with [2b] weights: half the
    sum of the two separate calls at 1e-6; the gradients are the separate calls' halves within 1e-6 of their scale."""
    rb = batches["mixed"]
    b, first, second = rb.b, OnDevice(rb, gpu), OnDevice(rb, gpu)
    with torch.no_grad():
        second.cur.add_(0.01).mul_(1.1)
    w1, w2 = per_mesh_weights(b), (150.0, 10.0, 75.0)
    l1, l2 = first.loss(on_device(w1, gpu)), second.loss(w2)
    (l1 + l2).backward()
    prev = torch.cat((first.prev.detach(), second.prev.detach())).requires_grad_(True)
    cur = torch.cat((first.cur.detach(), second.cur.detach())).requires_grad_(True)
    faces = torch.cat((first.faces, second.faces + rb.vt))
    csr = ragged.csr_from_faces(torch.cat((rb.adj_faces, rb.adj_faces + rb.vt)).to(gpu), 2 * rb.vt)
    stacked = tuple(torch.tensor(list(a) + [c] * b, dtype=torch.float32, device=gpu) for a, c in zip(w1, w2))
    both = utils.ragged_stage_regularisers(prev, cur, faces, torch.cat((first.face_mesh, second.face_mesh + b)),
                                           torch.cat((first.vert_mesh, second.vert_mesh + b)), csr, 2 * b, *stacked)
    both.backward()
    want = 0.5 * (l1.item() + l2.item())
    assert abs(both.item() - want) <= 1e-6 * abs(want), (both.item(), want)
    for got, halves in ((cur.grad, (first.cur.grad, second.cur.grad)), (prev.grad, (first.prev.grad, second.prev.grad))):
        ref = 0.5 * torch.cat(halves)
        assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


@pytest.mark.parametrize("name", ["mixed", "edge-cut"])
def test_ragged_calc_edge_against_float64_and_without_an_adjacency(gpu, batches, name):
    """The mean over the meshes of ref_ops.calc_edge in float64 at 1e-6, its gradient inside the per-element bounds; the node holds
    no adjacency tensor, no vertex ids and no previous positions."""
    rb = batches[name]
    weights = (0.0, 0.0, 1.0)
    want = sum(float(ref_ops.calc_edge(rb.cur[rb.vids[m]].double()[None], rb.local_faces[m])) for m in range(rb.b)) / rb.b
    exact, mass, floor = (union_chain(rb, weights, GOUT, absolute=a, ulps=u) for a, u in ((False, False), (True, False), (True, True)))
    assert abs(float(exact["value"]) - want) <= 1e-12 * want
    corners = max(int(np.bincount(f.reshape(-1).numpy()).max()) for f in rb.local_faces)
    verts = rb.cur.to(gpu).requires_grad_(True)
    loss = utils.ragged_calc_edge(verts, rb.faces.to(gpu), rb.face_mesh.to(gpu), rb.b)
    saved = loss.grad_fn.saved_tensors
    assert saved[0] is None and saved[4] is None and all(t is None for t in saved[6:10])
    (loss * GOUT).backward()
    assert abs(loss.item() - want) <= 1e-6 * want, (loss.item(), want)
    rows_close(verts.grad.cpu().numpy(), exact["grad_edge"].numpy(), mass["grad_edge"].numpy(), (corners + 8) * 2.0 ** -24,
               "ragged_calc_edge " + name, floor["grad_edge"].numpy(), ROW_FLOOR_ULPS)


def test_two_runs_give_the_same_bits(gpu, batches):
    rb = batches["edge-cut"]
    runs = []
    for _ in range(2):
        d = OnDevice(rb, gpu)
        loss = d.loss(on_device(per_mesh_weights(rb.b), gpu))
        loss.backward()
        runs.append((loss.detach(), d.cur.grad, d.prev.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_a_mesh_without_members_is_nan_and_ids_outside_the_batch_have_no_term(gpu, batches):
    """b one larger than the ids present (a mesh without a vertex and without a face): NaN.  A mesh whose faces are left out at an
    edge weight that is not 0: NaN; at weight 0 for that mesh: finite.  A vertex and a face that carry the id b + 3: the value
    of the batch without their terms (float64, the vertex's position still in its neighbours' Laplacians), gradients to 1e-5 of
    their scale.  Nothing faults."""
    rb = batches["mixed"]
    d = OnDevice(rb, gpu)
    loss = d.loss(SCALAR_WEIGHTS, b=rb.b + 1)
    loss.backward()
    assert bool(torch.isnan(loss))
    keep = d.face_mesh != 1
    without = dict(faces=d.faces[keep].contiguous(), face_mesh=d.face_mesh[keep].contiguous())
    d.cur.grad = d.prev.grad = None
    loss = d.loss(SCALAR_WEIGHTS, **without)
    loss.backward()
    assert bool(torch.isnan(loss))
    w_edge = [300.0 if m != 1 else 0.0 for m in range(rb.b)]
    loss = d.loss(on_device((300.0, 20.0, w_edge), gpu), **without)
    want = float(union_chain(rb, (300.0, 20.0, w_edge), GOUT)["value"])
    assert abs(loss.item() - want) <= 1e-6 * abs(want), (loss.item(), want)
    # ids outside [0, b): the union's first vertex of mesh 2 and its first face
    v_out, f_out = int(rb.vids[2][7]), int((rb.face_mesh == 2).nonzero()[0])
    vert_mesh, face_mesh = rb.vert_mesh.clone(), rb.face_mesh.clone()
    vert_mesh[v_out], face_mesh[f_out] = rb.b + 3, rb.b + 3
    nv = torch.tensor([(vert_mesh == m).sum() for m in range(rb.b)] + [1], dtype=torch.float64)
    nf = torch.tensor([(face_mesh == m).sum() for m in range(rb.b)] + [1], dtype=torch.float64)
    in_v = ((vert_mesh < rb.b).double(), vert_mesh.clamp(max=rb.b))
    in_f = ((face_mesh < rb.b).double(), face_mesh.clamp(max=rb.b))
    w_lap, w_move, w_edge = SCALAR_WEIGHTS
    c64, p64 = rb.cur.double().requires_grad_(True), rb.prev.double().requires_grad_(True)
    lap = ref_ops.lap_info(p64 - c64, rb.union_adj().double())
    p1, p2, p3 = (c64[rb.faces[:, k]] for k in range(3))
    edges = ((p2 - p1) ** 2).sum(-1) + ((p3 - p1) ** 2).sum(-1) + ((p2 - p3) ** 2).sum(-1)
    want = ((in_v[0] / (rb.b * nv[in_v[1]]) * (w_lap * (lap ** 2).sum(-1) + w_move * ((p64 - c64) ** 2).sum(-1))).sum()
            + (in_f[0] * w_edge / (3.0 * rb.b * nf[in_f[1]]) * edges).sum())
    want.backward()
    whole = float(union_chain(rb, SCALAR_WEIGHTS, GOUT)["value"])
    assert abs(float(want.detach()) - whole) > 2e-5 * abs(whole)                      # the two terms are 20 bars wide in the value
    d.cur.grad = d.prev.grad = None
    loss = d.loss(SCALAR_WEIGHTS, vert_mesh=vert_mesh.to(gpu), face_mesh=face_mesh.to(gpu))
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - float(want.detach())) <= 1e-6 * abs(float(want.detach())), (loss.item(), float(want.detach()))
    for got, ref in ((d.cur.grad, c64.grad), (d.prev.grad, p64.grad)):
        assert float((got.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_forward_and_backward_capture_in_one_graph_and_replay_on_new_positions(gpu, batches):
    """No host read once the caches are warm: forward and backward are captured in one torch.cuda.graph and replayed on
    positions copied into the captured tensors; value and gradients equal the eager call's on those positions."""
    rb = batches["mixed"]
    d = OnDevice(rb, gpu)
    weights = on_device(per_mesh_weights(rb.b), gpu)
    d.loss(weights).backward()                                   # fills the counts, the table and the vertex -> corner lists
    torch.cuda.synchronize()
    d.cur.grad = d.prev.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = d.loss(weights)
        loss.backward()
    moved = OnDevice(rb, gpu)
    with torch.no_grad():
        moved.cur.mul_(1.05).add_(0.02)
        moved.prev.mul_(0.97)
        d.cur.copy_(moved.cur)
        d.prev.copy_(moved.prev)
    graph.replay()
    torch.cuda.synchronize()
    eager = moved.loss(weights, faces=d.faces, face_mesh=d.face_mesh, vert_mesh=d.vert_mesh, csr=d.csr)
    eager.backward()
    assert torch.equal(loss.detach(), eager.detach()) and bool(torch.isfinite(eager))
    assert torch.equal(d.cur.grad, moved.cur.grad) and torch.equal(d.prev.grad, moved.prev.grad)


def test_csr_from_faces_equals_the_dense_route_and_from_faces_is_unchanged(gpu, batches):
    """rowptr, col and inv_deg of ragged.csr_from_faces equal those of layers.adjacency_csr on the dense adjacency of "mixed";
    RaggedMeshBatch.from_faces hands out what csr_from_faces builds from the concatenated face lists."""
    rb = batches["mixed"]
    got = ragged.csr_from_faces(rb.adj_faces.to(gpu), rb.vt)
    dense = layers.adjacency_csr(rb.union_adj().to(gpu))
    assert isinstance(got, layers._Csr) and got.nv == rb.vt
    for field in ("rowptr", "col", "inv_deg"):
        assert torch.equal(getattr(got, field), getattr(dense, field)), field
    assert int((got.rowptr[1:] - got.rowptr[:-1]).max()) == 33
    normalised = layers.adjacency_csr(utils.normalize_adj(rb.union_adj().to(gpu)))
    assert torch.equal(got.val, normalised.val) and torch.equal(got.val_t, normalised.val_t)
    lists = [torch.from_numpy(f).to(gpu) for _, f in (meshgen.icosphere(0), meshgen.icosphere(1))]
    batch = ragged.RaggedMeshBatch.from_faces([rb.cur[rb.vids[m]].to(gpu) for m in (0, 1)], lists)
    same = ragged.csr_from_faces(torch.cat((lists[0], lists[1] + 12)), 54)
    for field in ("rowptr", "col", "val", "rowptr_t", "col_t", "val_t", "inv_deg"):
        assert torch.equal(getattr(batch.csr, field), getattr(same, field)), field
    block = torch.block_diag(utils.calc_adj(lists[0]), utils.calc_adj(lists[1]))
    for field, want in (("rowptr", layers.adjacency_csr(block).rowptr), ("col", layers.adjacency_csr(block).col),
                        ("val", layers.adjacency_csr(utils.normalize_adj(block.clone())).val)):
        assert torch.equal(getattr(batch.csr, field), want), field
