"""CPU: the float64 references of the non-finite tests (tests/test_nonfinite_gpu.py).

ref_ops.zero_n_layer and helpers.block64 aggregate with the reference's dense `adj @ support` by default; there 0 * NaN is NaN,
so one NaN reaches every vertex of the aggregated slice.  The kernels sum a row's stored entries only, which is what
ref_ops.sparse_aggregate restates:

* on finite inputs the two forms agree to 1e-12 of scale (float64 round-off of a sum of at most 33 terms);
* on planted inputs the dense form's non-finite set CONTAINS the sparse form's: the reference never reports a finite number
  where the sparse form reports a non-finite one;
* helpers.nonfinite_close refuses each of the three things it is there to refuse."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from geometrics_amd import meshgen, models
from helpers import block192_case, block192_fixture, block192_parameters, block64, golden, nonfinite_close
from oracle import ref_ops

NAN, INF = float("nan"), float("inf")


def _adjacency(name):
    if name == "random48":          # the graph without a table of tests/test_aggregate_route_gpu.py, row-normalised
        g = torch.Generator(device="cpu").manual_seed(48)
        dense = (torch.rand(48, 48, generator=g) < 0.5).float()
        dense.fill_diagonal_(1.0)
        return ref_ops.normalize_adj(dense).double()
    faces = golden("adj_482")["faces"] if name == "template482" else meshgen.icosphere(2)[1]
    return ref_ops.normalize_adj(ref_ops.calc_adj(torch.from_numpy(np.ascontiguousarray(faces)).long())).double()


def _layer_operands(adj, cin, c, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(2, adj.shape[0], cin, generator=g, dtype=torch.float64)
    w = torch.randn(cin, c, generator=g, dtype=torch.float64) / cin ** 0.5
    bias = torch.randn(c, generator=g, dtype=torch.float64)
    return x, w, bias


@pytest.mark.parametrize("mesh", ["ico162", "template482", "random48"])
@pytest.mark.parametrize("split,activation", [(3, F.relu), (10, F.elu)])
def test_sparse_aggregation_equals_the_dense_product_on_finite_inputs(mesh, split, activation):
    adj = _adjacency(mesh)
    assert int((adj != 0).sum(1).max()) <= 33
    x, w, bias = _layer_operands(adj, 24, 30, 3)
    outs = []
    for aggregate in (ref_ops.dense_aggregate, ref_ops.sparse_aggregate):
        leaf = x.clone().requires_grad_(True)
        out = ref_ops.zero_n_layer(leaf, adj, w, bias, split, activation, aggregate=aggregate)
        out.backward(torch.cos(out.detach()))
        outs.append((out.detach(), leaf.grad))
    for dense, sparse in zip(*outs):
        assert float((dense - sparse).abs().max()) <= 1e-12 * float(dense.abs().max())
    assert torch.equal(ref_ops.zero_n_layer(x, adj, w, bias, split, activation), outs[0][0])     # dense is the default


def _small_block():
    g = block192_fixture("ico162_bn")
    inp = block192_case(g)
    block = block192_parameters(models.BatchMeshDeformationBlock(195, int(g["nv"])), g).train()
    return block, torch.from_numpy(inp["features"]).double(), torch.from_numpy(inp["pooled"]).double(), torch.from_numpy(g["adj"])


def test_block64_sparse_equals_block64_dense_on_finite_inputs():
    block, feats, pooled, adj = _small_block()
    with torch.no_grad():
        dense = block64(block, feats, pooled, adj)[:2]
        sparse = block64(block, feats, pooled, adj, aggregate=ref_ops.sparse_aggregate)[:2]
    for d, s in zip(dense, sparse):
        assert float((d - s).abs().max()) <= 1e-12 * float(d.abs().max())


@pytest.mark.parametrize("value", [NAN, INF, -INF])
@pytest.mark.parametrize("column", [0, 20])
def test_the_dense_forms_non_finite_set_contains_the_sparse_forms(value, column):
    """One planted input element.  The layer: the sparse form's non-finite rows are the planted vertex and the rows that hold
    it (aggregated columns) -- not every row, as under the dense product.  Two layers of the block: the same, ring by ring."""
    adj = _adjacency("template482")
    x, w, bias = _layer_operands(adj, 24, 30, 4)
    x[1, 7, column] = value
    dense = ref_ops.zero_n_layer(x, adj, w, bias, 3, F.relu)
    sparse = ref_ops.zero_n_layer(x, adj, w, bias, 3, F.relu, aggregate=ref_ops.sparse_aggregate)
    bad_d, bad_s = ~torch.isfinite(dense), ~torch.isfinite(sparse)
    assert bool((bad_d | ~bad_s).all()) and bool(bad_s.any())
    assert not bool(bad_s[0].any())                                                        # the other mesh is untouched
    holders = (adj[:, 7] != 0).nonzero().flatten().tolist()
    assert sorted(bad_s[1, :, :10].any(-1).nonzero().flatten().tolist()) == sorted(holders)
    assert bad_s[1, :, 10:].any(-1).nonzero().flatten().tolist() == [7]
    if value != value:                                                                        # 0 * NaN: every row of the mesh
        assert bool(bad_d[1, :, :10].all())
    finite = ~bad_d
    assert float((dense[finite] - sparse[finite]).abs().max()) <= 1e-12 * float(sparse[~bad_s].abs().max())


def test_block64_dense_non_finite_set_contains_the_sparse_one():
    block, feats, pooled, adj = _small_block()
    pooled = pooled.clone()
    pooled[2, 40, 5] = NAN
    with torch.no_grad():
        dense = block64(block, feats, pooled, adj)[:2]
        sparse = block64(block, feats, pooled, adj, aggregate=ref_ops.sparse_aggregate)[:2]
    for d, s in zip(dense, sparse):
        assert bool((~torch.isfinite(d) | torch.isfinite(s)).all()) and not bool(torch.isfinite(d).any())


def test_nonfinite_close_refuses_what_it_is_there_to_refuse():
    want = np.array([1.0, NAN, INF, -INF, 0.0])
    mass = np.array([1.0, 0.0, 0.0, 0.0, 0.0])
    ok = np.array([1.0 + 1e-7, NAN, INF, -INF, 0.0], np.float32)
    nonfinite_close(ok, want, mass, 1e-6, "ok")
    with pytest.raises(AssertionError, match="finite on one side only"):
        nonfinite_close(np.array([1.0, 0.0, INF, -INF, 0.0], np.float32), want, mass, 1e-6, "a scrubbed NaN")
    with pytest.raises(AssertionError, match="finite on one side only"):
        nonfinite_close(np.array([NAN, NAN, INF, -INF, 0.0], np.float32), want, mass, 1e-6, "a NaN too many")
    swapped = np.array([1.0, INF, NAN, -INF, 0.0], np.float32)
    with pytest.raises(AssertionError, match="NaN differs"):
        nonfinite_close(swapped, want, mass, 1e-6, "kinds swapped")
    nonfinite_close(swapped, want, mass, 1e-6, "kinds swapped, mask only", kinds=False)
    with pytest.raises(AssertionError, match="-Inf differs|\\+Inf differs"):
        nonfinite_close(np.array([1.0, NAN, -INF, INF, 0.0], np.float32), want, mass, 1e-6, "signs swapped")
    with pytest.raises(AssertionError, match="worst element"):
        nonfinite_close(np.array([1.001, NAN, INF, -INF, 0.0], np.float32), want, mass, 1e-6, "a finite element off")
    with pytest.raises(AssertionError, match="worst element"):
        nonfinite_close(np.array([1.0, NAN, INF, -INF, 1e-3], np.float32), want, mass, 1e-6, "a saturated output off")
