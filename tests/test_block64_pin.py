"""CPU: the float64 restatement of the mesh deformation block (helpers.block64, reference models.py:237-297) that the fused
block's GPU tests compare against, pinned to the reference's own results:

* tests/golden/block192.npz (the reference block at width 192, run in float64): every stored output, gradient, running
  statistic and eval-mode output within the fixture's fp32 storage rounding, every seeded-weight checksum of a full tensor
  within 1e-9 -- both sides are float64;
* tests/golden/deformation_block_v162.npz (hidden 24, run by the reference in float32): at that fixture's own bars.

And the vertex-count guard of the per-vertex BatchNorm, which raises on the host like nn.BatchNorm1d."""
import numpy as np
import pytest
import torch

from geometrics_amd import models
from helpers import (BLOCK192_CASES, block192_case, block192_fixture, block192_parameters, block192_stored, block64, golden,
                     weighted_checksum)


@pytest.mark.parametrize("case", BLOCK192_CASES)
def test_block64_against_the_block192_fixture(case):
    g = block192_fixture(case)
    inp = block192_case(g)
    block = block192_parameters(models.BatchMeshDeformationBlock(195, int(g["nv"])), g).train()
    b = int(g["batch"])
    feats, pooled = (torch.from_numpy(inp[k]).double().requires_grad_(True) for k in ("features", "pooled"))
    adj = torch.from_numpy(g["adj"])
    stats, pre = [], []
    out_f, coords, params = block64(block, feats, pooled, adj, relu=bool(g["relu"]), stats=stats, pre=pre)
    if bool(g["relu"]):      # (the ReLU cases' inputs keep every pre-activation off the kink: make_golden.py _off_the_kink)
        assert min(float(y.abs().min()) for y in pre) >= float(g["kink"])
    g_f, g_c = (torch.from_numpy(inp[k]).double() for k in ("g_features", "g_coords"))
    ((out_f * g_f).sum() + (coords * g_c).sum()).backward()
    # running statistics after one step from (0, 1): nn.BatchNorm1d's update with the unbiased variance
    n = b * 192
    m = [float(x) for x in g["bn_momentum"][:13]]
    full = {"features": out_f, "coords": coords, "grad.features": feats.grad, "grad.pooled": pooled.grad,
            "running_mean": torch.stack([m[i] * mean for i, (mean, _) in enumerate(stats)]),
            "running_var": torch.stack([(1 - m[i]) + m[i] * var * n / (n - 1) for i, (_, var) in enumerate(stats)])}
    full.update({"grad." + k: p.grad for k, p in params.items() if not k.startswith("bn14")})
    assert all(params[k].grad is None for k in params if k.startswith("bn14"))
    if "eval.coords" in g:
        with torch.no_grad():
            running = {i: (full["running_mean"][i - 1], full["running_var"][i - 1]) for i in range(1, 14)}
            full["eval.features"], full["eval.coords"], _ = block64(block, feats.detach(), pooled.detach(), adj, relu=True,
                                                                    running=running)
    full = {k: v.detach().numpy() for k, v in full.items()}
    assert sorted(full) == list(g["ck_names"])
    stored = block192_stored(g, full)
    assert set(stored) == {k for k in g if k in stored} and len(stored) >= 15
    for key, got in stored.items():
        want = g[key].astype(np.float64)
        assert want.shape == got.shape, key
        # the fixture holds the float64 results rounded to fp32: within half an fp32 ulp (+ 1e-9 of the tensor's scale)
        bound = 2.0 ** -24 * np.abs(want) * (1 + 2.0 ** -22) + 1e-9 * np.abs(want).max()
        worst = float((np.abs(got - want) / bound).max())
        assert worst <= 1.0, "%s: %.2fx the fp32 storage rounding" % (key, worst)
    for name, (want, scale) in zip(g["ck_names"], g["ck"]):
        got = weighted_checksum(str(name), full[str(name)])[0]
        assert abs(got - want) <= 1e-9 * scale, "%s: checksum off by %.2e of its scale" % (name, abs(got - want) / scale)


def test_block64_against_the_hidden24_fixture():
    """deformation_block_v162.npz: the reference block (hidden 24) run in float32 -- at that fixture's bars (test_ops_parity_gpu.py
    test_deformation_block_matches_reference_fixture)."""
    g = golden("deformation_block_v162")

    def close(got, want, rtol):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        err = np.abs(got - want).max()
        assert err <= rtol * np.abs(want).max(), "max abs err %g vs tol %g" % (err, rtol * np.abs(want).max())
    block = models.BatchMeshDeformationBlock(32, 162, hidden=24, output_features=3)
    state = {k[len("state."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("state.")}
    block.load_state_dict(state, strict=True)
    block.train()
    feats, pooled = (torch.from_numpy(g[k]).double().requires_grad_(True) for k in ("features", "pooled"))
    stats = []
    out_f, coords, params = block64(block, feats, pooled, torch.from_numpy(g["adj"]), stats=stats)
    close(out_f.detach(), g["out_features"], 2e-5)
    close(coords.detach(), g["coords"], 2e-5)
    ((out_f * torch.from_numpy(g["g_features"]).double()).sum() + (coords * torch.from_numpy(g["g_coords"]).double()).sum()).backward()
    close(feats.grad, g["grad_features"], 2e-4)
    close(pooled.grad, g["grad_pooled"], 2e-4)
    for k in [k[len("grad."):] for k in g if k.startswith("grad.")]:
        close(params[k].grad, g["grad." + k], 3e-4)
    n = 3 * 24
    for i in (1, 13):
        mean, var = stats[i - 1]
        close(0.1 * mean, g["after.bn%d.running_mean" % i], 1e-5)
        close(0.9 + 0.1 * var * n / (n - 1), g["after.bn%d.running_var" % i], 1e-5)


def test_vertex_batchnorm_raises_on_another_vertex_count():
    """nn.BatchNorm1d(162) given 482-vertex activations raises; so does VertexBatchNorm, on the host, before any route is
    chosen (on the device the kernels would index the 162-entry statistics by vertices up to 481)."""
    x = torch.randn(2, 482, 6)
    with pytest.raises(RuntimeError, match="running_mean should contain"):
        torch.nn.BatchNorm1d(162)(x)
    bn = models.VertexBatchNorm(162).train()
    with pytest.raises(RuntimeError, match="running_mean should contain 482 elements not 162"):
        bn(x, relu=True)
    assert bn._pending_batches == 0 and bool((bn.running_mean == 0).all()) and bool((bn.running_var == 1).all())
