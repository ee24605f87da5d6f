"""CPU: the ragged stage regularisers without a GPU -- the two entry points declared, exported and refusing bad arguments
before any launch; the union-order float64 chain of ragged_reg_helpers against the oracle's restatements per mesh, the same
chain in fp32 under half of every bound and a chain that loses ONE term outside them; the per-mesh counts and the coefficient
table (torch ops) against their numpy restatement."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from geometrics_amd import _header, _lib, ragged
from ragged_reg_helpers import BATCHES, SCALAR_WEIGHTS, bounds, coefficients, counts_and_coefficients, mixed, reference_value, union_chain
from test_ops_parity_gpu import stage_regulariser_outputs_close

P = 8        # any non-null address: validation never dereferences
FWD, BWD, BLOCKS = "geom_ragged_regularisers_fwd_f32", "geom_ragged_regularisers_bwd_f32", "geom_ragged_regularisers_blocks"
EINVAL = _header.CONSTANTS["EINVAL"]
GOUT = 0.7


def per_mesh_weights(b):
    """[b] weights that differ per mesh and include a 0 in every row."""
    return ([300.0 * (m + 1) for m in range(b - 1)] + [0.0], [0.0] + [20.0 + 5.0 * m for m in range(b - 1)],
            [300.0 if m != b // 2 else 0.0 for m in range(b)])


def test_the_ragged_regulariser_symbols_are_declared_and_exported_and_the_abi_version_stands():
    L = _lib.lib()
    assert L.geom_abi_version() == 16 == _lib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout
    exported = {line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in "Tt"}
    for name in (FWD, BWD, BLOCKS):
        assert name in _lib.declared_symbols() and name in exported, name
    for name in (FWD, BWD):
        restype, argtypes = _header.PROTOTYPES[name]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p        # a code back, the stream last
    shared = ["b", "nv", "prev", "cur", "nf", "faces", "vert_mesh", "face_mesh", "coef", "nnz", "rowptr", "col", "inv_deg"]
    assert [p for p, _, _ in _header.PARAMETERS[FWD]] == shared + ["lapd", "partial", "stream"]
    assert [p for p, _, _ in _header.PARAMETERS[BWD]] == shared + ["vf_ptr", "vf_item", "lapd", "gout", "grad_prev", "grad_cur", "stream"]
    # eight lanes per vertex or one per face, whichever are more, in workgroups of 256
    assert [L.geom_ragged_regularisers_blocks(nv, nf) for nv, nf in ((698, 1396), (32, 256), (32, 257), (1, 0), (96, 789))] == [22, 1, 2, 1, 4]


def test_the_ragged_forward_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(b=2, nv=4, prev=P, cur=P, nf=4, faces=P, vert_mesh=P, face_mesh=P, coef=P, nnz=9, rowptr=P, col=P, inv_deg=P, lapd=P, partial=P)
    call = lambda **kw: L.geom_ragged_regularisers_fwd_f32(*{**ok, **kw}.values(), None)
    for size in ("b", "nv", "nf", "nnz"):
        assert call(**{size: -1}) == EINVAL, size
    for pointer in ("prev", "cur", "vert_mesh", "face_mesh", "coef", "col", "inv_deg", "lapd", "partial"):
        assert call(**{pointer: None}) == EINVAL, pointer
    assert call(b=(2 ** 31 - 1) // 3 + 1) == _header.CONSTANTS["ETOOBIG"]       # 3 b table entries are counted in an int
    assert call(b=0) == 0 and call(nv=0) == 0                                    # nothing to do
    assert call(b=0, prev=None, cur=None, faces=None, vert_mesh=None, face_mesh=None, coef=None, rowptr=None, col=None, inv_deg=None,
                lapd=None, partial=None) == 0


def test_the_ragged_backward_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(b=2, nv=4, prev=P, cur=P, nf=4, faces=P, vert_mesh=P, face_mesh=P, coef=P, nnz=9, rowptr=P, col=P, inv_deg=P, vf_ptr=P,
              vf_item=P, lapd=P, gout=P, grad_prev=P, grad_cur=P)
    call = lambda **kw: L.geom_ragged_regularisers_bwd_f32(*{**ok, **kw}.values(), None)
    for size in ("b", "nv", "nf", "nnz"):
        assert call(**{size: -1}) == EINVAL, size
    for pointer in ("prev", "cur", "vert_mesh", "face_mesh", "coef", "col", "inv_deg", "vf_ptr", "vf_item", "lapd", "gout", "grad_cur"):
        assert call(**{pointer: None}) == EINVAL, pointer
    assert call(rowptr=None) == EINVAL                                           # grad_prev without the terms prev is in
    assert call(b=0) == 0 and call(nv=0) == 0
    assert call(nv=0, prev=None, cur=None, faces=None, vert_mesh=None, face_mesh=None, coef=None, rowptr=None, col=None, inv_deg=None,
                vf_ptr=None, vf_item=None, lapd=None, gout=None, grad_prev=None, grad_cur=None) == 0


@pytest.mark.parametrize("name", sorted(BATCHES))
@pytest.mark.parametrize("per_mesh", [False, True])
def test_union_chain_is_the_oracles_and_fp32_is_inside_the_bounds_and_a_lost_term_outside(name, per_mesh):
    rb = BATCHES[name]()
    per_mesh = per_mesh and rb.b > 1           # (one mesh: the scalar weights again)
    weights = per_mesh_weights(rb.b) if per_mesh else SCALAR_WEIGHTS
    exact, mass, floor, rtol = bounds(rb, weights, GOUT)        # (holds the float64 chain to ref_ops per mesh at 1e-12)
    keys = ("lapd", "grad_cur", "grad_prev")
    numpy = lambda out: {k: out[k].numpy() for k in keys}
    host = union_chain(rb, weights, GOUT, dtype=torch.float32)
    stage_regulariser_outputs_close(numpy(host), exact, mass, floor, rtol, name + " (fp32 on the host)", 0.5)
    assert abs(float(host["value"]) - float(exact["value"])) <= 1e-6 * abs(float(exact["value"]))
    # the vertex with the smallest gradient (of a mesh whose Laplacian weight is not 0) loses its last neighbour
    strength = exact["grad_cur"].abs().sum(1)
    live = [m for m in range(rb.b) if not per_mesh or weights[0][m] != 0.0]
    target = min(live, key=lambda m: float(strength[rb.vids[m]].min()))
    v = int(strength[rb.vids[target]].argmin())

    def lose_entry(m, adj, faces, coef):
        if m == target:
            others = adj[v].nonzero().flatten()
            adj = adj.clone()
            adj[v, int(others[others != v][-1])] = 0.0
        return adj, faces, coef
    with pytest.raises(AssertionError):
        stage_regulariser_outputs_close(numpy(union_chain(rb, weights, GOUT, dtype=torch.float32, edit=lose_entry)), exact, mass, floor,
                                        rtol, name)
    # the last face of a mesh with an edge term is not gathered
    edged = [m for m in range(rb.b) if rb.local_faces[m].shape[0] and (not per_mesh or weights[2][m] != 0.0)][-1]
    with pytest.raises(AssertionError):
        stage_regulariser_outputs_close(numpy(union_chain(rb, weights, GOUT, dtype=torch.float32,
                                                          edit=lambda m, adj, faces, coef: (adj, faces[:-1] if m == edged else faces, coef))),
                                        exact, mass, floor, rtol, name)
    if rb.b > 1:                # one mesh's coefficients replaced by another's
        donor = coefficients(rb, weights, 0)
        assert donor != coefficients(rb, weights, 1)
        with pytest.raises(AssertionError):
            stage_regulariser_outputs_close(numpy(union_chain(rb, weights, GOUT, dtype=torch.float32,
                                                              edit=lambda m, adj, faces, coef: (adj, faces, donor if m == 1 else coef))),
                                            exact, mass, floor, rtol, name)


def test_the_unions_counts_in_place_of_each_meshs_give_another_value():
    """What the GPU test asserts first: on "mixed" the value of a kernel that ignores the ids is far from the exact one."""
    rb = mixed()
    exact = float(reference_value(rb, SCALAR_WEIGHTS)[0].detach())
    ignoring = float(reference_value(rb, SCALAR_WEIGHTS, union_counts=True)[0].detach())
    assert abs(ignoring - exact) > 1e-2 * abs(exact), (ignoring, exact)


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_counts_and_coefficient_table_equal_their_numpy_restatement(name):
    rb = BATCHES[name]()
    b = rb.b + 1                                                 # the last mesh has no member at all
    ids_v, ids_f = rb.vert_mesh.clone(), rb.face_mesh.clone()
    ids_v[::17] = b + 3                                          # members of no mesh, on either side of the range
    ids_v[5::29] = -2
    ids_f[::13] = b
    if rb.b > 1:
        ids_f[ids_f == 1] = 0                                    # a mesh with vertices and no face
    weights = (300.0, [0.0] + [20.0] * (b - 1), [300.0] * (b - 1) + [0.0])
    want_v, want_f, want = counts_and_coefficients(ids_v.numpy(), ids_f.numpy(), b, weights)
    got_ids, got_v = ragged.mesh_counts(ids_v, b)
    assert got_ids.dtype == torch.int32 and got_ids.is_contiguous() and got_v.dtype == torch.int64
    np.testing.assert_array_equal(got_v.numpy(), want_v)
    np.testing.assert_array_equal(ragged.mesh_counts(ids_f, b)[1].numpy(), want_f)
    inside = (ids_v >= 0) & (ids_v < b)
    np.testing.assert_array_equal(got_ids[inside].numpy(), ids_v[inside].numpy())
    assert not ((got_ids[~inside] >= 0) & (got_ids[~inside] < b)).any()
    assert ragged.mesh_counts(ids_v, b)[0] is got_ids                       # cached per tensor object and version ...
    assert ragged.mesh_counts(ids_v.clone(), b)[0] is not got_ids
    assert ragged.mesh_counts(ids_v.to(torch.int32), b)[1].tolist() == want_v.tolist()
    tensors = tuple(torch.tensor(w, dtype=torch.float32) if isinstance(w, list) else w for w in weights)
    fm, vm, coef = ragged.regulariser_tables(ids_f, ids_v, b, *tensors)
    assert coef.dtype == torch.float32 and coef.shape == (3, b) and vm is got_ids
    np.testing.assert_array_equal(coef.numpy(), want)                       # NaN == NaN here; one rounding from float64
    assert np.isnan(want[:2, -1]).all() and want[2, -1] == 0.0 and want[1, 0] == 0.0
    if rb.b > 1:
        assert np.isnan(want[2, 1])
    assert ragged.regulariser_tables(ids_f, ids_v, b, *tensors)[2] is coef  # ... and so is the table
    assert ragged.regulariser_tables(ids_f, ids_v, b, 1.0, tensors[1], tensors[2])[2] is not coef
    ids_v[0] = 0                                                            # an in-place change drops both
    assert ragged.mesh_counts(ids_v, b)[0] is not got_ids
    assert ragged.regulariser_tables(ids_f, ids_v, b, *tensors)[2] is not coef
    # the edge term alone: no vertex ids, the first two rows 0
    edge_only = ragged.regulariser_tables(ids_f, None, b, 0.0, 0.0, 1.0)
    assert edge_only[1] is None and not edge_only[2][:2].any()
    np.testing.assert_array_equal(edge_only[2][2].numpy(), counts_and_coefficients(ids_v.numpy(), ids_f.numpy(), b, (0.0, 0.0, 1.0))[2][2])
