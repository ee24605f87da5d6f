"""Helpers of the eval-mode deformation block tests: tests/golden/block192_eval.npz (tests/golden/make_block192_eval.py)."""
import numpy as np
import torch

from geometrics_amd import models
from helpers import fill_block_parameters, golden, seeded_input

EVAL_CASES = ("eval482_b1", "eval482_b40", "eval162_b3")


def eval_fixture(case):
    """One case of tests/golden/block192_eval.npz without the case prefix, with its mesh's dense fp32 adjacency `adj`, the
    inputs regenerated from the seed (checked against the stored sums) and `running` = {layer: (mean, var)}."""
    g = golden("block192_eval")
    out = {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(case + ".")}
    mesh = str(out["mesh"])
    out.update({k[len(mesh) + 1:]: v for k, v in g.items() if k.startswith(mesh + ".")})
    nv, b, seed = int(out["nv"]), int(out["batch"]), int(out["seed"])
    adj = np.zeros((nv, nv), np.float32)
    adj[out["adj_rows"].astype(np.int64), out["adj_cols"].astype(np.int64)] = out["adj_vals"]
    out["adj"] = adj
    out["features"] = seeded_input([seed, 0], (b, nv, 3))
    out["pooled"] = seeded_input([seed, 1], (b, nv, 192))
    for k in ("features", "pooled"):
        assert float(out[k].astype(np.float64).sum()) == float(out["in_ck." + k]), k
    out["running"] = {i: (out["running_mean"][i - 1], out["running_var"][i - 1]) for i in range(1, 14)}
    return out


def eval_block(g, device="cpu"):
    """The project's block with a case's parameters, BatchNorm eps and running statistics, in eval mode."""
    block = fill_block_parameters(models.BatchMeshDeformationBlock(195, int(g["nv"])), int(g["seed"])).to(device)
    with torch.no_grad():
        for i in range(1, 15):
            bn = getattr(block, "bn%d" % i)
            bn.eps = float(g["bn_eps"][i - 1])
            if i < 14:
                bn.running_mean.copy_(torch.from_numpy(g["running_mean"][i - 1]))
                bn.running_var.copy_(torch.from_numpy(g["running_var"][i - 1]))
    return block.eval()
