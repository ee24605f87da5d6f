"""Adaptive face splitting for a ragged batch held as one union mesh (utils.ragged_adj_init / ragged_active_faces /
ragged_calc_curve / ragged_split_info on the ragged launches of csrc/face_split.hip): against the per-mesh calls, against the
existing kernels run on the union as one mesh with its dense matrices, and through the functions that take the result.

The union is five icospheres (1050 vertices, 2080 faces: every new launch spans at least five chunks of 256 items and meshes
straddle their boundaries), once concatenated and once with vertices and faces shuffled.  Comparisons are torch.equal /
np.array_equal: the union's launches are the per-mesh launches' arithmetic."""
import functools

import numpy as np
import pytest
import torch

import face_split_helpers as fh
import helpers
import ragged_split_helpers as rh
from geometrics_amd import layers, meshgen, models, ragged, utils

C_SMALL, C_WIDE = 5, 192
CSR_ARRAYS = ("rowptr", "col", "val", "val_t")


def dev(a, device, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t.requires_grad_(True) if grad else t


def host(t):
    return t.detach().cpu().numpy()


def union_info(u, device):
    return utils.ragged_adj_init(dev(u.faces, device), dev(u.vert_mesh, device), u.b)


def dense_info(faces, device):
    info = utils.adj_init(dev(faces, device))
    info["face_list"] = utils.calc_face_list(info["faces"])
    return info


def tables(info):
    """The union's index tables as numpy arrays: (faces, face_list, face_mesh, vert_mesh)."""
    return tuple(host(info[k]) for k in ("faces", "face_list", "face_mesh", "vert_mesh"))


def per_mesh_selection(info, verts, angle, device):
    """[the union positions calc_curve selects on mesh m ALONE, in its order] for every mesh: the mesh is the union's tables
    restricted and relabelled by rank, its positions mapped back through the union rows of the mesh."""
    out = []
    for m in range(info["b"]):
        vids, _, rows, faces_m, fl_m = rh.restrict(m, *tables(info))
        own = {"faces": dev(faces_m, device), "face_list": dev(fl_m, device)}
        out.append(rows[host(utils.calc_curve(dev(verts[vids], device), own, angle))])
    return out


def selection_equals_the_per_mesh_calls(info, verts, angle, device):
    splitting, counts = utils.ragged_calc_curve(dev(verts, device), info, angle)
    want = per_mesh_selection(info, verts, angle, device)
    assert splitting.dtype == counts.dtype == torch.int64 and splitting.is_cuda and counts.is_cuda
    assert np.array_equal(host(splitting), np.concatenate(want)), "the union's list is not the per-mesh lists, mesh after mesh"
    assert host(counts).tolist() == [len(w) for w in want]
    return host(splitting), want


# ------------------------------------------------------------------------------------------------------ 1: selection ----
@pytest.mark.gpu
@pytest.mark.parametrize("shuffled", (False, True), ids=("concatenated", "shuffled"))
def test_selection_is_each_mesh_s_own(gpu, shuffled):
    """At the threshold angle every mesh has at least 3 faces above it and the union's list is the per-mesh calc_curve results
    mapped to union positions, mesh after mesh; at the fallback angle the un-jittered mesh (fewer than 3 above) takes ITS OWN
    three most curved faces -- ties to the lower positions -- while the others keep their hits.  Both angles stand clear of every
    face's float64 curvature by more than its bound (rh.angles).  Two runs give the same outputs."""
    u = rh.union(shuffled)
    info = union_info(u, gpu)
    face_list = host(info["face_list"])
    assert np.array_equal(host(info["face_mesh"]), u.vert_mesh[u.faces[:, 1]]) and info["csr"].nv == len(u.verts)
    deg, margin = rh.degrees64(u.verts, u.faces, face_list)
    mesh = host(info["face_mesh"])[face_list[:, 0, 2]]
    threshold, fallback = rh.angles()
    for angle in (threshold, fallback):
        assert rh.clear_of(angle, deg, margin)
        got, want = selection_equals_the_per_mesh_calls(info, u.verts, angle, gpu)
        hits = [np.flatnonzero((mesh == m) & (deg > angle)) for m in range(u.b)]
        for m in range(u.b):
            if angle == threshold or m != rh.SMOOTH:
                assert len(hits[m]) >= 3 and np.array_equal(want[m], hits[m]), (angle, m)      # the float64 decision, ascending
            else:
                rows = np.flatnonzero(mesh == m)
                third = np.sort(deg[rows])[-3]          # (faces closer than their bounds may change places in fp32)
                assert len(hits[m]) < 3 and len(set(want[m])) == 3 and set(want[m]) <= set(rows)
                assert (deg[want[m]] >= third - 2.0 * margin[rows].max()).all(), "not the mesh's three largest curvatures"
        again, counts = utils.ragged_calc_curve(dev(u.verts, gpu), info, angle)
        assert np.array_equal(host(again), got)


@pytest.mark.gpu
def test_selection_ties_go_to_the_lower_positions_and_rows_of_no_mesh_are_never_selected(gpu):
    """The un-jittered icosphere's largest curvature is shared by many faces with the same bits: its fallback is the three
    LOWEST positions among them, in ascending order.  With b = 3 the rows of meshes 3 and 4 belong to no mesh."""
    u = rh.union(True)
    info = union_info(u, gpu)
    _, fallback = rh.angles()
    splitting, counts = utils.ragged_calc_curve(dev(u.verts, gpu), info, fallback)
    start = int(host(counts)[:rh.SMOOTH].sum())
    own = host(splitting)[start:start + 3]
    from geometrics_amd import ops
    curv = host(ops.face_curvature(dev(u.verts, gpu), info["faces"], info["face_list"]))
    rows = np.flatnonzero(host(info["face_mesh"])[host(info["face_list"])[:, 0, 2]] == rh.SMOOTH)
    order = rows[np.lexsort((rows, -curv[rows]))]          # the kernel's own bits: largest first, the lower position on ties
    assert len(np.unique(curv[rows])) < len(rows), "the un-jittered icosphere has no two faces with the same curvature"
    assert host(counts)[rh.SMOOTH] == 3 and np.array_equal(own, order[:3])
    fewer = dict(info, b=3)
    got, got_counts = utils.ragged_calc_curve(dev(u.verts, gpu), fewer, fallback)
    assert np.array_equal(host(got), host(splitting)[:int(host(counts)[:3].sum())]) and np.array_equal(host(got_counts), host(counts)[:3])


@pytest.mark.gpu
def test_degenerate_faces_are_never_selected_and_a_mesh_without_three_curvatures_raises(gpu):
    u = rh.union(False)
    info = union_info(u, gpu)
    verts = u.verts.copy()
    face = int(np.flatnonzero(u.vert_mesh[u.faces[:, 0]] == 1)[11])        # a face of mesh 1: two of its corners in one place
    verts[u.faces[face, 2]] = verts[u.faces[face, 0]]
    from geometrics_amd import ops
    curv = host(ops.face_curvature(dev(verts, gpu), info["faces"], info["face_list"]))
    without_normal = set(np.flatnonzero(np.isnan(curv)).tolist())
    assert 4 <= len(without_normal) < 320
    for angle in (1.0, 179.0):                  # nearly every face above the angle; none above it (five fallbacks)
        got, _ = selection_equals_the_per_mesh_calls(info, verts, angle, gpu)
        assert len(got) >= 3 * u.b and not (set(got.tolist()) & without_normal)
    # a tetrahedron with two coincident vertices has no face with a curvature: the call raises as calc_curve does
    tetra = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0]], np.float32), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64))
    two = rh.join([rh.meshes()[0], tetra], shuffled=False)
    with pytest.raises(RuntimeError, match="1 of the 2 meshes have fewer than 3 faces with a curvature"):
        utils.ragged_calc_curve(dev(two.verts, gpu), union_info(two, gpu), 20.0)


# ------------------------------------------------------------- 2: the split against the existing kernels on the union ----
@functools.lru_cache(maxsize=None)
def threshold_list():
    device = torch.device("cuda:0")
    u = rh.union(True)
    return host(utils.ragged_calc_curve(dev(u.verts, device), union_info(u, device), rh.angles()[0])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("c", (C_SMALL, C_WIDE))
@pytest.mark.parametrize("which", ("none", "one", "selected"))
def test_split_equals_split_info_on_the_union_as_one_mesh(gpu, which, c):
    """At 1050 vertices the dense matrices are affordable: utils.split_info on the union as ONE mesh (the one-workgroup index
    launch) and ragged_split_info agree on faces, face_list, the four CSR arrays, the new vertices and features, and both input
    gradients under a seeded cotangent -- for no face, one face and ragged_calc_curve's list."""
    u = rh.union(True)
    positions = {"none": np.zeros(0, np.int64), "one": np.array([1234], np.int64), "selected": threshold_list()}[which]
    s, nv = len(positions), len(u.verts)
    assert which != "selected" or s > 3 * u.b
    features = helpers.seeded_input([31, c], (nv, c))
    cot_v, cot_f = dev(helpers.seeded_input([32, c], (nv + s, 3)), gpu), dev(helpers.seeded_input([33, c], (nv + s, c)), gpu)
    results = []
    for make, split in ((union_info, lambda i, v, f, p: utils.ragged_split_info(i, v, f, p)),
                        (lambda u_, d: dense_info(u_.faces, d), lambda i, v, f, p: utils.split_info(i, v, f, p, p.numel()))):
        v, f = dev(u.verts, gpu, grad=True), dev(features, gpu, grad=True)
        new_info, v2, f2 = split(make(u, gpu), v, f, dev(positions, gpu))
        torch.autograd.backward((v2, f2), (cot_v, cot_f))
        results.append((new_info, v2.detach(), f2.detach(), v.grad, f.grad))
    (ours, *got), (theirs, *want) = results
    assert "adj" not in ours and "adj_orig" not in ours and ours["b"] == u.b
    assert torch.equal(ours["faces"], theirs["faces"]) and torch.equal(ours["face_list"], theirs["face_list"])
    assert ours["faces"].shape == (len(u.faces) + 3 * s, 3) and ours["face_list"].shape == (len(u.faces) + 2 * s, 3, 3)
    csr = layers.registered_csr(theirs["adj"])
    for name in CSR_ARRAYS:
        assert torch.equal(getattr(ours["csr"], name), getattr(csr, name)), name
    for name, a, b_ in zip(("verts", "features", "grad verts", "grad features"), got, want):
        assert a.shape == b_.shape and torch.equal(a, b_), name
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[3]).all()


# ------------------------------------------------------------------------ 3: the split against each mesh alone, chained ----
ROUNDS = 2


@functools.lru_cache(maxsize=None)
def union_chain(shuffled):
    """Two chained rounds on the union: select, split, move the vertices by a seeded displacement, select, split.  Per round a
    dict of what went in, what came out and the input gradients under a seeded cotangent."""
    device = torch.device("cuda:0")
    u = rh.union(shuffled)
    info = union_info(u, device)
    v, f = u.verts, helpers.seeded_input([41, int(shuffled)], (len(u.verts), C_SMALL))
    out = []
    for r in range(ROUNDS):
        vd, fd = dev(v, device, grad=True), dev(f, device, grad=True)
        splitting, counts = utils.ragged_calc_curve(vd, info, rh.angles()[0])
        new_info, v2, f2 = utils.ragged_split_info(info, vd, fd, splitting)
        cot_v, cot_f = helpers.seeded_input([42, r], tuple(v2.shape)), helpers.seeded_input([43, r], tuple(f2.shape))
        torch.autograd.backward((v2, f2), (dev(cot_v, device), dev(cot_f, device)))
        move = helpers.seeded_input([44, r], tuple(v2.shape), scale=0.01)
        out.append(dict(info=info, new_info=new_info, splitting=host(splitting), counts=host(counts), verts=host(v2), features=host(f2),
                        grad_verts=host(vd.grad), grad_features=host(fd.grad), cot_v=cot_v, cot_f=cot_f, move=move))
        info, v, f = new_info, host(v2) + move, host(f2)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shuffled", (False, True), ids=("concatenated", "shuffled"))
def test_the_union_restricted_to_a_mesh_is_that_mesh_split_alone(gpu, shuffled):
    """After each of two chained rounds, the union's result restricted to mesh m and relabelled by rank -- faces, face_list,
    the ids, the CSR rows, the vertices, the features, both gradients -- equals the chain utils.calc_curve + utils.split_info
    runs on mesh m ALONE (which sees of the union only its own restriction of the seeded displacement and cotangents)."""
    chain = union_chain(shuffled)
    u = rh.union(shuffled)
    for m in range(u.b):
        vids, _, rows, faces_m, fl_m = rh.restrict(m, *tables(chain[0]["info"]))
        info = dense_info(faces_m, gpu)
        assert np.array_equal(host(info["face_list"]), fl_m), "calc_face_list on the union is not calc_face_list on the mesh"
        v, f = u.verts[vids], helpers.seeded_input([41, int(shuffled)], (len(u.verts), C_SMALL))[vids]
        for r, rnd in enumerate(chain):
            what = "mesh %d round %d" % (m, r + 1)
            vd, fd = dev(v, gpu, grad=True), dev(f, gpu, grad=True)
            selected = utils.calc_curve(vd, info, rh.angles()[0])
            new_info, v2, f2 = utils.split_info(info, vd, fd, selected, selected.numel())
            start = int(rnd["counts"][:m].sum())
            assert np.array_equal(rnd["splitting"][start:start + rnd["counts"][m]], rows[host(selected)]), what + ": selection"
            new_tables = tables(rnd["new_info"])
            new_vids, new_fids, new_rows, new_faces_m, new_fl_m = rh.restrict(m, *new_tables)
            assert np.array_equal(new_faces_m, host(new_info["faces"])), what + ": faces"
            assert np.array_equal(new_fl_m, host(new_info["face_list"])), what + ": face_list"
            assert len(new_vids) == v2.shape[0] and np.array_equal(new_vids[:len(vids)], vids), what + ": vert_mesh"
            faces_u, _, face_mesh_u, vert_mesh_u = new_tables
            assert all(np.array_equal(face_mesh_u, vert_mesh_u[faces_u[:, k]]) for k in range(3)), what + ": face_mesh"
            ours, theirs = rnd["new_info"]["csr"], layers.registered_csr(new_info["adj"])
            got = rh.restrict_csr(new_vids, len(vert_mesh_u), *(host(getattr(ours, n)) for n in CSR_ARRAYS))
            for name, a in zip(CSR_ARRAYS, got):
                assert np.array_equal(a, host(getattr(theirs, name))), what + ": csr " + name
            torch.autograd.backward((v2, f2), (dev(rnd["cot_v"][new_vids], gpu), dev(rnd["cot_f"][new_vids], gpu)))
            for name, a, b_ in (("verts", rnd["verts"][new_vids], v2), ("features", rnd["features"][new_vids], f2),
                                ("grad verts", rnd["grad_verts"][vids], vd.grad), ("grad features", rnd["grad_features"][vids], fd.grad)):
                assert np.array_equal(helpers.bits(a), helpers.bits(host(b_))), what + ": " + name
            if m == 0 and r == 0:       # and the reference's rules written out row by row
                restated = fh.split_tables_restated(faces_m, fl_m, host(selected), host(info["adj_orig"]))
                assert np.array_equal(new_faces_m, restated[0]) and np.array_equal(new_fl_m, restated[1])
                dense = np.zeros_like(restated[2])
                rowptr, col, val, _ = got
                dense[np.repeat(np.arange(len(new_vids)), np.diff(rowptr)), col] = val
                assert np.array_equal(helpers.bits(dense), helpers.bits(restated[2])), what + ": the normalised adjacency"
            info, vids, rows = new_info, new_vids, new_rows
            v, f = host(v2) + rnd["move"][new_vids], host(f2)


# ---------------------------------------------------------------------------------------- 4: what takes the new info ----
@pytest.mark.gpu
def test_the_new_info_serves_the_ragged_losses_the_pooling_and_the_block(gpu):
    """After two rounds new_info['csr'] is ragged.csr_from_faces of the active faces, array for array, and the ragged surface
    loss, the ragged stage regularisers, the ragged pooling and MeshDeformationBlock take the new info: finite values, finite
    gradients."""
    rnd = union_chain(True)[-1]
    info, b = rnd["new_info"], rh.B
    n = info["vert_mesh"].numel()
    faces, face_mesh = utils.ragged_active_faces(info)
    assert utils.ragged_active_faces(info)[0] is faces and faces.shape == (info["face_list"].shape[0], 3)
    assert torch.equal(faces, info["faces"][info["face_list"][:, 0, 2]]) and torch.equal(face_mesh, info["face_mesh"][info["face_list"][:, 0, 2]])
    rebuilt = ragged.csr_from_faces(faces, n)
    for name in CSR_ARRAYS:
        assert torch.equal(getattr(info["csr"], name), getattr(rebuilt, name)), name
    finished = layers.adjacency_csr(info["csr"])          # the derived tables, made at first use
    assert finished is info["csr"] and finished.nv == n and finished.ell_w == rebuilt.ell_w and torch.equal(finished.inv_deg, rebuilt.inv_deg)
    verts = dev(rnd["verts"], gpu, grad=True)
    prev = dev(rnd["verts"] + rnd["move"], gpu)
    gt = dev(np.stack([meshgen.gt_cloud(1, 200, first=m)[0] for m in range(b)]), gpu)
    loss = utils.ragged_point_to_surface(verts, faces, face_mesh, gt, num=64)
    reg = utils.ragged_stage_regularisers(prev, verts, faces, face_mesh, info["vert_mesh"], info["csr"], b, 1.0, 0.5, 0.25)
    maps = [dev(helpers.seeded_input([51, l], (b, 8, d, d)), gpu, grad=True) for l, d in enumerate((16, 8))]
    cams = torch.tensor([[30.0 * m, 20.0 + 5.0 * m, 1.0 + 0.05 * m] for m in range(b)], device=gpu)
    pooled = utils.ragged_pooling(maps, verts, info["vert_mesh"], cams)
    features = dev(helpers.seeded_input([52], (n, 8)), gpu, grad=True)
    torch.manual_seed(53)
    block = models.MeshDeformationBlock(8 + 16, hidden=24).to(gpu)
    feats, coords = block(features, pooled, info["csr"])
    assert pooled.shape == (n, 16) and feats.shape == (n, 24) and coords.shape == (n, 3)
    total = loss + reg + feats.sum() + coords.sum()
    total.backward()
    assert all(bool(torch.isfinite(t).all()) for t in (loss, reg, pooled, feats, coords))
    for name, t in (("verts", verts), ("features", features), ("map 0", maps[0]), ("map 1", maps[1]), ("weight", block.gc1.weight1)):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any()), name


@pytest.mark.gpu
def test_the_split_is_captured_in_a_graph_without_a_host_read(gpu):
    """Nothing in ragged_split_info reads the host (a read would end the capture with an error): the call is recorded in a HIP
    graph, replayed on vertices changed in place, and gives what the eager call gives on them.  The csr it hands over holds the
    six arrays alone; layers.adjacency_csr completes it at first use to what layers.csr_from_parts makes of the arrays."""
    u = rh.union(True)
    info = union_info(u, gpu)
    verts, features = dev(u.verts, gpu), dev(helpers.seeded_input([71], (len(u.verts), 8)), gpu)
    splitting = dev(threshold_list(), gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        utils.ragged_split_info(info, verts, features, splitting)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        new_info, v2, f2 = utils.ragged_split_info(info, verts, features, splitting)      # recorded, not executed
    verts.mul_(1.5)
    graph.replay()
    torch.cuda.synchronize()
    want_info, want_v, want_f = utils.ragged_split_info(info, verts, features, splitting)
    assert torch.equal(v2, want_v) and torch.equal(f2, want_f) and not hasattr(new_info["csr"], "ell_w")
    for key in ("faces", "face_list", "face_mesh", "vert_mesh"):
        assert torch.equal(new_info[key], want_info[key]), key
    arrays = [getattr(want_info["csr"], name) for name in ("rowptr", "col", "val", "rowptr_t", "col_t", "val_t")]
    finished, want = layers.adjacency_csr(new_info["csr"]), layers.csr_from_parts(*arrays)
    assert finished is new_info["csr"] and finished.ell_w == want.ell_w and finished.nv == v2.shape[0] and finished.symmetric_structure
    for name in CSR_ARRAYS + ("inv_deg",) + (("ell_col", "ell_val") if finished.ell_w else ()):
        assert torch.equal(getattr(finished, name), getattr(want, name)), name


# ------------------------------------------------------------------------------------------------- 5: no dense matrix ----
@pytest.mark.gpu
def test_no_dense_matrix_is_allocated(gpu):
    """A union of 16 icosphere(3): 10 272 vertices, where ONE dense fp32 [n,n] matrix is 422 MB.  Over a ragged_split_info call
    the peak of allocated memory rises by less than a quarter of that (the outputs are O(n): a few MB).  A condition, not a
    measurement."""
    u = rh.join(rh.meshes((3,) * 16, smooth=-1), shuffled=False)
    assert len(u.verts) == 10272
    info = union_info(u, gpu)
    verts, features = dev(u.verts, gpu), dev(helpers.seeded_input([61], (len(u.verts), 8)), gpu)
    splitting = torch.arange(0, info["face_list"].shape[0], 3, device=gpu)
    one_dense = 4 * len(u.verts) ** 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    new_info, v2, f2 = utils.ragged_split_info(info, verts, features, splitting)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak allocated memory rose by %.1f MB (one dense matrix: %.0f MB)" % (rise / 2 ** 20, one_dense / 2 ** 20))
    assert rise < one_dense / 4
    assert v2.shape[0] == len(u.verts) + splitting.numel() == new_info["vert_mesh"].numel() == new_info["csr"].rowptr.numel() - 1
    counts = torch.bincount(new_info["vert_mesh"], minlength=16)
    assert counts.sum() == v2.shape[0] and bool((counts >= 642).all())
