"""Generate tests/golden/block192_eval.npz: the reference's BatchMeshDeformationBlock(195, V) (hidden 192) in eval mode under
no_grad, in FLOAT64, with non-trivial running statistics -- what the driver's validation and evaluation run
(GEOMetrics.py:187-247, 286-362).

    python tests/golden/make_block192_eval.py

`import make_golden` provides the stubs the reference's modules need, the reference's path and save(); its __main__ guard
keeps it from writing anything.  Per case:

  * the block: fill_block_parameters(seed), the case's BatchNorm eps;
  * inputs: features [B,V,3] = seeded_input([seed, 0]), pooled [B,V,192] = seeded_input([seed, 1]);
  * running statistics: the float64 batch statistics (mean, biased variance) of the same block in training mode on a second
    seeded batch of 16 ([seed, 10], [seed, 11]); then, rng [seed, 12], layer by layer, every vertex's variance times
    exp(U(ln 0.25, ln 4)) and its mean shifted by U(-0.5, 0.5) * the std of that batch; rounded to fp32 and stored;
  * stored: weighted checksums of the full features and coordinates, 24 sampled (mesh, vertex) rows of the features (vertices
    0 and V-1 and three of each one's neighbours among them), the coordinates of the first and the last mesh.

The maker asserts, and stores, (1) every layer's share of positive pre-activations in [0.05, 0.95] (both ReLU branches are
exercised) and (2) a float32 evaluation of the same reference block within 5e-6 of scale of the float64 result (a quarter of
the 2e-5 bar the tests hold the kernels to)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stubs, reference path, save())

sys.path.insert(0, os.path.join(make_golden.ROOT, "tests"))
import helpers  # noqa: E402

# case -> (mesh, batch, seed, {layer: BatchNorm eps})
CASES = {"eval482_b1": ("uv_sphere_482", 1, 1930, {}),
         "eval482_b40": ("uv_sphere_482", 40, 1931, {}),
         "eval162_b3": ("icosphere_162", 3, 1932, {5: 1e-3, 13: 1e-4})}
ROWS = 24
STATS_BATCH = 16


def _maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def running_statistics(block, nv, seed, adj):
    """([13, V] mean, [13, V] var) fp32, as the module docstring says."""
    feats = torch.from_numpy(helpers.seeded_input([seed, 10], (STATS_BATCH, nv, 3))).double()
    pooled = torch.from_numpy(helpers.seeded_input([seed, 11], (STATS_BATCH, nv, 192))).double()
    stats = []
    with torch.no_grad():
        helpers.block64(block, feats, pooled, adj, relu=True, stats=stats)
    rng = np.random.default_rng([seed, 12])
    means, variances = [], []
    for mean, var in stats:
        mean, var = mean.numpy().astype(np.float64), var.numpy().astype(np.float64)
        factor = np.exp(rng.uniform(np.log(0.25), np.log(4.0), nv))
        shift = rng.uniform(-0.5, 0.5, nv) * np.sqrt(var)
        means.append((mean + shift).astype(np.float32))
        variances.append((var * factor).astype(np.float32))
    return np.stack(means), np.stack(variances)


def make_block192_eval():
    import models as ref_models                      # the reference's models.py
    assert ref_models.__file__.startswith(make_golden.REF)
    arrays = {}
    for mesh in ("uv_sphere_482", "icosphere_162"):
        V, Fc = make_golden.meshgen.uv_sphere() if mesh == "uv_sphere_482" else make_golden.meshgen.icosphere(2)
        adj = make_golden.ref_utils.adj_init(make_golden.t(Fc))["adj"].numpy()
        r, c = np.nonzero(adj)
        arrays.update({"%s.adj_rows" % mesh: r.astype(np.int16), "%s.adj_cols" % mesh: c.astype(np.int16),
                       "%s.adj_vals" % mesh: adj[r, c].astype(np.float32)})
    for case, (mesh, batch, seed, eps_of) in CASES.items():
        nv = 482 if mesh == "uv_sphere_482" else 162
        r, c = arrays["%s.adj_rows" % mesh].astype(np.int64), arrays["%s.adj_cols" % mesh].astype(np.int64)
        adj = np.zeros((nv, nv), np.float32)
        adj[r, c] = arrays["%s.adj_vals" % mesh]
        A = torch.from_numpy(adj).double()
        eps = np.full(14, 1e-5)
        for layer, value in eps_of.items():
            eps[layer - 1] = value
        block = helpers.fill_block_parameters(ref_models.BatchMeshDeformationBlock(195, nv), seed)
        for i in range(1, 15):
            getattr(block, "bn%d" % i).eps = float(eps[i - 1])
        rm, rv = running_statistics(block, nv, seed, A)
        inp = {"features": helpers.seeded_input([seed, 0], (batch, nv, 3)),
               "pooled": helpers.seeded_input([seed, 1], (batch, nv, 192))}
        out = dict(mesh=np.array(mesh), batch=np.int64(batch), nv=np.int64(nv), seed=np.int64(seed), bn_eps=eps,
                   running_mean=rm, running_var=rv)
        out.update({"in_ck." + k: np.float64(v.astype(np.float64).sum()) for k, v in inp.items()})

        def evaluate(dtype):
            blk = block.to(dtype).eval()
            with torch.no_grad():
                for i in range(1, 14):
                    bn = getattr(blk, "bn%d" % i)
                    bn.running_mean.copy_(torch.from_numpy(rm[i - 1]))
                    bn.running_var.copy_(torch.from_numpy(rv[i - 1]))
                f, p = (torch.from_numpy(inp[k]).to(dtype) for k in ("features", "pooled"))
                feats, coords = blk(f, p, A.to(dtype))
            return feats.double().numpy(), coords.double().numpy()
        feats32, coords32 = evaluate(torch.float32)
        feats, coords = evaluate(torch.float64)
        err32 = max(_maxrel(feats32, feats), _maxrel(coords32, coords))
        assert err32 <= 5e-6, "%s: float32 is %.2e of scale from float64" % (case, err32)
        # every layer's share of positive pre-activations (the float64 restatement with the same statistics)
        pre = []
        running = {i: (rm[i - 1].astype(np.float64), rv[i - 1].astype(np.float64)) for i in range(1, 14)}
        with torch.no_grad():
            f64, c64, _ = helpers.block64(block, *(torch.from_numpy(inp[k]).double() for k in ("features", "pooled")), A,
                                          relu=True, running=running, pre=pre)
        positive = np.array([float((y > 0).double().mean()) for y in pre])
        assert ((positive >= 0.05) & (positive <= 0.95)).all(), "%s: positive shares %s" % (case, positive)
        out.update(float32_err=np.float64(err32), positive_share=positive)
        rng = np.random.default_rng([seed, 7])
        ends = [0, nv - 1]
        rings = [np.array([j for j in np.nonzero(adj[e])[0] if j != e]) for e in ends]
        rows_v = ends + [int(ring[k * len(ring) // 3]) for ring in rings for k in range(3)]
        rest = np.setdiff1d(np.arange(nv), rows_v)
        rows_v += [int(v) for v in rng.choice(rest, ROWS - len(rows_v), replace=False)]
        rows_b = rng.integers(0, batch, ROWS)
        rows_b[0], rows_b[1] = 0, batch - 1
        rows_v, rows_b = np.array(rows_v, np.int32), rows_b.astype(np.int32)
        meshes = np.array([0, batch - 1], np.int32)
        out.update(rows_v=rows_v, rows_b=rows_b, meshes=meshes,
                   features_rows=feats[rows_b, rows_v].astype(np.float32), coords=coords[meshes].astype(np.float32),
                   ck_names=np.array(["coords", "features"]),
                   ck=np.stack([helpers.weighted_checksum("coords", coords), helpers.weighted_checksum("features", feats)]))
        print("%-12s float32 %.2e of scale, positive shares %.2f .. %.2f" % (case, err32, positive.min(), positive.max()))
        arrays.update({"%s.%s" % (case, k): v for k, v in out.items()})
    make_golden.save("block192_eval", **arrays)


if __name__ == "__main__":
    make_block192_eval()
