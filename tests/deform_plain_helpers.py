"""Shared by tests/golden/make_plain_block.py and the tests of the BatchNorm-free deformation block
(models.MeshDeformationBlock, layers.Image_ZERON_GCNGCN; reference models.py:138-201 on old_GEOMetrics/layers.py:106-149):
the cases of tests/golden/plain_block.npz, their adjacencies, parameters and inputs regenerated from seeds, what the fixture
stores of a case's full results, and the adjacencies of the launch tests."""
import zlib

import numpy as np

from helpers import golden, seeded_input, weighted_checksum

ROWS = 24            # sampled rows of the 192-wide tensors
WROWS = 16           # sampled rows of the weight gradients of gc1, gc2, gc7, gc13
WLAYERS = (1, 2, 7, 13)
HIDDEN = tuple(range(1, 14))

# case -> (adjacency, ReLU, seed); "layer40": ONE Image_ZERON_GCNGCN(40, 48) layer with ReLU instead of the block
BLOCK_CASES = {"sphere482": ("uv_sphere_482", True, 4101), "split181": ("split_ico1_r2", True, 4102),
               "split181_smooth": ("split_ico1_r2", False, 4103)}
LAYER_CASE = ("layer40", "split_ico1_r2", 4104, 40, 48)

# the bars of the fp32 routes against float64 (tests/test_deform_gpu.py's), as fractions of a tensor's largest magnitude
FORWARD_BAR, GRADIENT_BAR = 2e-5, 5e-5


def coo_dense(rows, cols, vals, nv):
    adj = np.zeros((nv, nv), np.float32)
    adj[np.asarray(rows, np.int64), np.asarray(cols, np.int64)] = vals
    return adj


def split_adjacency(fixture, prefix):
    """The dense fp32 adjacency a committed face-split fixture stores after round / list `prefix`."""
    g = golden(fixture)
    return coo_dense(g[prefix + ".adj.rows"], g[prefix + ".adj.cols"], g[prefix + ".adj.vals"], int(g[prefix + ".nv"]))


def case_adjacency(name, g=None):
    """Dense fp32 [V,V] adjacency of a fixture case: the split mesh from its own committed fixture, the UV sphere from the
    COO arrays plain_block.npz stores (g = the loaded fixture)."""
    if name == "split_ico1_r2":
        return split_adjacency("split_ico1_two_rounds", "r2")
    g = golden("plain_block") if g is None else g
    return coo_dense(g[name + ".adj_rows"], g[name + ".adj_cols"], g[name + ".adj_vals"], int(g[name + ".nv"]))


def fill_plain_parameters(module, seed):
    """Deterministic parameters at the reference's init scale (old_GEOMetrics/layers.py:124-133: weight1 ~ U(+-0.6 * 6 /
    sqrt(in + out)), bias ~ U(+-0.1)), one numpy stream per parameter name: the reference's classes and the project's get the
    same values whatever their dtype."""
    import torch
    with torch.no_grad():
        for name, p in sorted(module.named_parameters()):
            rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
            bound = 3.6 / np.sqrt(p.shape[0] + p.shape[1]) if p.dim() == 2 else 0.1
            p.copy_(torch.from_numpy(rng.uniform(-bound, bound, tuple(p.shape)).astype(np.float32)))
    return module


def case_inputs(seed, nv, width_in=3, width_pooled=192, width_out=192, g=None, case=None):
    """fp32 inputs and cotangents of a case regenerated from its seed (checked against the fixture's float64 checksums when
    g / case are given): features [V,width_in], pooled [V,width_pooled], g_features [V,width_out], g_coords [V,3]."""
    shapes = dict(features=(nv, width_in), pooled=(nv, width_pooled), g_features=(nv, width_out), g_coords=(nv, 3))
    out = {}
    for k, (name, shape) in enumerate(sorted(shapes.items())):
        out[name] = seeded_input([seed, k], shape)
        key = "%s.in_ck.%s" % (case, name)
        if g is not None and key in g:
            assert float(out[name].astype(np.float64).sum()) == float(g[key]), name
    return out


def sampled_rows(seed, nv, adj):
    """ROWS vertices: the first, the last, the longest row, then a seeded draw."""
    rng = np.random.default_rng([seed, 7])
    fixed = list(dict.fromkeys([0, nv - 1, int((adj != 0).sum(1).argmax())]))
    rest = np.setdiff1d(np.arange(nv), fixed)
    return np.array(fixed + [int(v) for v in rng.choice(rest, ROWS - len(fixed), replace=False)], np.int32)


def weight_rows(seed, layer, n_in):
    rng = np.random.default_rng([seed, 11, layer])
    return np.concatenate(([0, 1, 2, n_in - 1], rng.choice(np.arange(3, n_in - 1), WROWS - 4, replace=False))).astype(np.int32)


def block_full(out_f, coords, feats, pooled, block):
    """name -> tensor of every output and gradient of a block case after backward()."""
    full = {"features": out_f, "coords": coords, "grad.features": feats.grad, "grad.pooled": pooled.grad}
    for name, p in block.named_parameters():
        full["grad." + name] = p.grad
    return {k: v.detach().double().cpu().numpy() for k, v in full.items()}


def block_stored(full, rows_v, wrows):
    """What plain_block.npz keeps of a block case's full results: sampled rows of the 192-wide tensors, the [V,3] tensors
    whole, the bias gradients stacked, the head's gradients, sampled rows of four weight gradients."""
    rv = np.asarray(rows_v, np.int64)
    out = {"features_rows": full["features"][rv], "coords": full["coords"], "grad.features": full["grad.features"],
           "grad.pooled_rows": full["grad.pooled"][rv],
           "grad.gc_bias": np.stack([full["grad.gc%d.bias" % i] for i in HIDDEN]),
           "grad.gc15.bias": full["grad.gc15.bias"], "grad.gc15.weight1": full["grad.gc15.weight1"]}
    for i in WLAYERS:
        out["grad.gc%d.weight1_rows" % i] = full["grad.gc%d.weight1" % i][np.asarray(wrows[i], np.int64)]
    return out


def checksums(full):
    names = sorted(full)
    return names, np.stack([weighted_checksum(n, full[n]) for n in names])


def errors_against(g, case, full):
    """name -> error of `full` (a case's full results, numpy) against the fixture, as a fraction of the stored tensor's
    largest magnitude: every stored array element by element, and every full tensor through its weighted checksum."""
    rows_v = g[case + ".rows_v"]
    wrows = {i: g["%s.wrows.gc%d" % (case, i)] for i in WLAYERS}
    errs = {}
    for name, got in block_stored(full, rows_v, wrows).items():
        want = g["%s.%s" % (case, name)].astype(np.float64)
        errs[name] = float(np.abs(got - want).max() / np.abs(want).max())
    for name, (want, scale) in zip(g[case + ".ck_names"], g[case + ".ck"]):
        errs["ck." + str(name)] = float(abs(weighted_checksum(str(name), full[str(name)])[0] - want) / scale)
    return errs


def bar_of(g, case, name):
    """The bar of a stored quantity: the project's (forward 2e-5, gradients 5e-5 of scale) unless the maker stored its own
    (`bar.<name>`: four times the fp32 reference's error where that missed a quarter of the project's)."""
    key = "%s.bar.%s" % (case, name)
    if g is not None and key in g:
        return float(g[key])
    plain = name[3:] if name.startswith("ck.") else name
    return FORWARD_BAR if plain in ("features", "features_rows", "coords") else GRADIENT_BAR


def run_block(block, inputs, adj, relu, dtype, device="cpu"):
    """One forward + backward of `block` (the reference's class or the project's) on a case's inputs: its full results.  The
    ReLU of a smooth case is dropped the way the fixture's maker drops it: torch.nn.functional.relu becomes the identity
    (and geometrics_amd.deform.relu goes off for the fused route)."""
    import torch
    from geometrics_amd import deform
    feats, pooled = (torch.from_numpy(inputs[k]).to(device=device, dtype=dtype).requires_grad_(True) for k in ("features", "pooled"))
    g_f, g_c = (torch.from_numpy(inputs[k]).to(device=device, dtype=dtype) for k in ("g_features", "g_coords"))
    relu_fn, relu_flag = torch.nn.functional.relu, deform.relu
    if not relu:
        torch.nn.functional.relu = lambda x, inplace=False: x
        deform.relu = False
    try:
        out_f, coords = block(feats, pooled, adj)
        ((out_f * g_f).sum() + (coords * g_c).sum()).backward()
    finally:
        torch.nn.functional.relu, deform.relu = relu_fn, relu_flag
    return block_full(out_f, coords, feats, pooled, block)


# ---- the adjacencies of the launch tests ------------------------------------------------------------------------------------
def launch_adjacency(which):
    """(a) icosphere(1): 42 vertices, 3 row-blocks, the last of 10 rows, no overflow; (b) the UV sphere: 482, poles of 33, a
    last block of 2 rows; (c) split_ico1_two_rounds r2: 181, ell_w == 0, rows up to 21; (d) split_482_pole `pole`: 519, one
    row of 65.  Dense fp32 [V,V], rows normalised as the reference's normalize_adj does."""
    import torch
    from geometrics_amd import meshgen, utils
    if which in ("a", "b"):
        _, faces = meshgen.icosphere(1) if which == "a" else meshgen.uv_sphere()
        return utils.adj_init(torch.from_numpy(np.asarray(faces, np.int64)))["adj"].numpy().astype(np.float32)
    if which == "c":
        return split_adjacency("split_ico1_two_rounds", "r2")
    return split_adjacency("split_482_pole", "pole")
