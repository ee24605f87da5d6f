import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def golden_names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fill_parameters(module, seed, gain=2.0):
    """Deterministic parameter values independent of torch's RNG stream (so a fixture only stores the seed):
    matrices ~ U(+-gain/sqrt(sum(shape))), vectors ~ U(+-0.1), in sorted-name order."""
    import zlib

    import torch
    with torch.no_grad():
        for name, p in sorted(module.named_parameters()):
            rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
            bound = gain / np.sqrt(sum(p.shape)) if p.dim() >= 2 else 0.1
            p.copy_(torch.from_numpy(rng.uniform(-bound, bound, tuple(p.shape)).astype(np.float32)))
    return module


def fill_block_parameters(block, seed):
    """fill_parameters for a mesh deformation block (reference models.py:203-235) at the reference's own init scale
    (layers.py:99-105: weight1 [1, in, out] ~ U(+-0.3 * 6 / sqrt(in + 1)), bias ~ U(+-0.1)) and with non-trivial
    BatchNorm affine parameters: weight ~ U(0.5, 1.5), bias ~ U(-0.3, 0.3).  Same seed-per-name scheme: the block of the
    reference (nn.BatchNorm1d) and the project's get the same values whatever their dtype."""
    import zlib

    import torch
    with torch.no_grad():
        for name, p in sorted(block.named_parameters()):
            rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
            if name.endswith("weight1"):
                lo, hi = -1.8 / np.sqrt(p.shape[1] + p.shape[0]), 1.8 / np.sqrt(p.shape[1] + p.shape[0])
            elif name.startswith("bn"):
                lo, hi = (0.5, 1.5) if name.endswith("weight") else (-0.3, 0.3)
            else:
                lo, hi = -0.1, 0.1
            p.copy_(torch.from_numpy(rng.uniform(lo, hi, tuple(p.shape)).astype(np.float32)))
    return block


def seeded_input(seed, shape, scale=1.0):
    """A deterministic fp32 array ~ scale * N(0, 1) (numpy's generator, independent of torch's stream)."""
    return (np.random.default_rng(seed).standard_normal(tuple(shape)) * scale).astype(np.float32)


def checksum_weights(name, shape):
    """Seeded float64 weights in U(-1, 1) for the checksum of a tensor called `name`."""
    import zlib
    return np.random.default_rng([1920, zlib.crc32(name.encode())]).uniform(-1.0, 1.0, tuple(shape))


def weighted_checksum(name, t):
    """(sum(t * w), sum(|t| * |w|)) in float64, w = checksum_weights(name, t.shape): a change anywhere in t moves the first
    by its size times a weight of order one; the second is the scale the first is compared at."""
    t = np.asarray(t, np.float64)
    w = checksum_weights(name, t.shape)
    return np.array([(t * w).sum(), (np.abs(t) * np.abs(w)).sum()])


# ---- the mesh deformation block restated in float64 (reference models.py:237-297 on layers.py:107-116) --------------------
def bn64(z, gamma, beta, eps):
    """nn.BatchNorm1d(verts) on [B,V,C] in training mode, float64: one statistic per vertex over (B, C)."""
    mean = z.mean(dim=(0, 2), keepdim=True)
    var = ((z - mean) ** 2).mean(dim=(0, 2), keepdim=True)
    return (z - mean) / (var + eps).sqrt() * gamma.view(1, -1, 1) + beta.view(1, -1, 1), mean.flatten(), var.flatten()


def block64(block, feats, pooled, adj, relu=True, stats=None, running=None, pre=None, aggregate=None):
    """models.py:237-297 restated in float64 on the host (dense adjacency, torch ops): returns (features, coords, parameters)
    -- the parameters as float64 leaves, whose .grad a backward pass fills.  Each layer normalises with ITS BatchNorm's eps.
    stats (a list): receives every layer's batch statistics (mean, biased variance) in order.  running ({layer: (mean, var)}):
    eval mode -- those statistics normalise instead of the batch's.  pre (a list): receives every layer's pre-activation (what
    the ReLU is applied to).  aggregate: ref_ops.dense_aggregate (the default, the reference's product) or
    ref_ops.sparse_aggregate (the sum over a row's stored entries, which is what the kernels form)."""
    import torch
    from oracle import ref_ops
    aggregate = aggregate or ref_ops.dense_aggregate
    p = {k: v.detach().double().cpu().requires_grad_(v.requires_grad) for k, v in block.named_parameters()}
    adj = adj.double().cpu()

    def gc(i, x):
        sup = x @ p["gc%d.weight1" % i][0]
        k = sup.shape[-1] // 3
        return torch.cat((aggregate(adj, sup[..., :k]), sup[..., k:]), dim=-1) + p["gc%d.bias" % i]

    def layer(i, x):
        gamma, beta, eps = p["bn%d.weight" % i], p["bn%d.bias" % i], float(getattr(block, "bn%d" % i).eps)
        if running is not None:
            mean, var = (torch.as_tensor(t, dtype=torch.float64).view(1, -1, 1) for t in running[i])
            y = (gc(i, x) - mean) / (var + eps).sqrt() * gamma.view(1, -1, 1) + beta.view(1, -1, 1)
        else:
            y, mean, var = bn64(gc(i, x), gamma, beta, eps)
            if stats is not None:
                stats.append((mean.detach(), var.detach()))
        if pre is not None:
            pre.append(y.detach())
        return torch.relu(y) if relu else y
    f = torch.cat((feats, pooled), dim=-1)
    x = layer(1, f)
    x = layer(2, x)
    f = (f[..., :block.hidden] + x) / 2
    for i in (3, 5, 7, 9, 11):
        x = layer(i, f)
        x = layer(i + 1, x)
        f = (f + x) / 2
    x = layer(13, f)
    f = (f + x) / 2
    return f, gc(15, f), p


def block192_parameters(block, g):
    """A case's parameters on `block` (the reference's or the project's, any dtype): fill_block_parameters(seed), then the
    case's BatchNorm biases moved off the ReLU kink (bn_fix_layer / bn_fix_vertex / bn_fix_value: see make_golden.py
    make_block192) and its per-layer BatchNorm eps / momentum; checked against the fixture's checksums where it has them."""
    import torch
    fill_block_parameters(block, int(g["seed"]))
    with torch.no_grad():
        for layer, v, value in zip(g.get("bn_fix_layer", ()), g.get("bn_fix_vertex", ()), g.get("bn_fix_value", ())):
            getattr(block, "bn%d" % int(layer)).bias[int(v)] = float(value)
    for i in range(1, 15):
        bn = getattr(block, "bn%d" % i)
        bn.eps, bn.momentum = float(g["bn_eps"][i - 1]), float(g["bn_momentum"][i - 1])
    if "in_ck.params" in g:
        named = dict(block.named_parameters())
        assert sorted(named) == list(g["param_names"])
        assert [float(named[n].detach().double().sum()) for n in g["param_names"]] == list(g["in_ck.params"])
    return block


def block192_case(g):
    """Inputs of a case of tests/golden/block192.npz regenerated from its seeds, each checked against the fixture's float64
    checksum (a change in numpy's random stream fails here instead of comparing different inputs): dict of fp32 arrays
    features [B,V,3], pooled [B,V,192], g_features [B,V,192], g_coords [B,V,3]."""
    b, nv, seed = int(g["batch"]), int(g["nv"]), int(g["seed"])
    shapes = dict(features=(b, nv, 3), pooled=(b, nv, 192), g_features=(b, nv, 192), g_coords=(b, nv, 3))
    out = {}
    for k, (name, shape) in enumerate(sorted(shapes.items())):
        out[name] = seeded_input([seed, k], shape)
        if "in_ck." + name in g:
            assert float(out[name].astype(np.float64).sum()) == float(g["in_ck." + name]), name
    return out


BLOCK192_CASES = ("train482", "smooth482", "ico162_bn", "ico162_b24")


def block192_fixture(case):
    """One case of tests/golden/block192.npz as a dict without the case prefix, with its mesh's COO adjacency (adj_rows,
    adj_cols, adj_vals) and `adj` (the dense fp32 [V,V] matrix)."""
    g = golden("block192")
    out = {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(case + ".")}
    mesh = str(out["mesh"])
    out.update({k[len(mesh) + 1:]: v for k, v in g.items() if k.startswith(mesh + ".")})
    nv = int(out["nv"])
    adj = np.zeros((nv, nv), np.float32)
    adj[out["adj_rows"].astype(np.int64), out["adj_cols"].astype(np.int64)] = out["adj_vals"]
    out["adj"] = adj
    return out


def block192_stored(g, full):
    """The arrays block192.npz stores, taken out of a case's FULL results (numpy; keyed like the fixture's checksums:
    features, coords, grad.features, grad.pooled, grad.<parameter>, running_mean / running_var [13,V], eval.*) exactly as
    the fixture's maker takes them: (mesh, vertex) rows of the 192-wide tensors, two whole meshes of the [B,V,3] ones,
    sampled rows of four weight gradients, the rest in full; the 13 layers' vectors stacked."""
    rb, rv, m = g["rows_b"].astype(np.int64), g["rows_v"].astype(np.int64), g["meshes"].astype(np.int64)
    out = {"features_rows": full["features"][rb, rv], "coords": full["coords"][m], "grad.features": full["grad.features"][m],
           "grad.pooled_rows": full["grad.pooled"][rb, rv],
           "grad.gc_bias": np.stack([full["grad.gc%d.bias" % i] for i in range(1, 14)]),
           "grad.gc15.bias": full["grad.gc15.bias"], "grad.gc15.weight1": full["grad.gc15.weight1"],
           "grad.bn_weight": np.stack([full["grad.bn%d.weight" % i] for i in range(1, 14)]),
           "grad.bn_bias": np.stack([full["grad.bn%d.bias" % i] for i in range(1, 14)]),
           "running_mean": full["running_mean"], "running_var": full["running_var"]}
    for i in (1, 2, 7, 13):
        out["grad.gc%d.weight1_rows" % i] = full["grad.gc%d.weight1" % i][0][g["wrows.gc%d" % i].astype(np.int64)]
    if "eval.features" in full:
        out["eval.features_rows"] = full["eval.features"][rb, rv]
        out["eval.coords"] = full["eval.coords"][m]
    return out


def log_margin(what, err, bar):
    """err against its bar (both relative); appended to $GEOM_MARGIN_LOG when set (margins of a run, for the bounds)."""
    log = os.environ.get("GEOM_MARGIN_LOG")
    if log:
        with open(log, "a") as f:
            f.write("%s: %.3g (bar %g, %.3f of it)\n" % (what, err, bar, err / bar))
    return err <= bar


def tri_true_case(name):
    """Inputs of a tests/golden/tri_true_*.npz fixture, regenerated from their seeds (the fixture stores the expected
    per-point true squared distances + a checksum of the inputs): (verts [B,V,3], faces [F,3], points [B,N,3], true [B,N])."""
    from geometrics_amd import meshgen
    g = golden(name)
    V, F = meshgen.icosphere(int(g["level"]))
    first = int(g["first"]) if "first" in g else 0
    verts = meshgen.jittered_batch(V, int(g["batch"]), first=first)
    pts = meshgen.gt_cloud(int(g["batch"]), int(g["num"]), first=first, cube=bool(g["cube"]))
    assert float(verts.astype(np.float64).sum() + pts.astype(np.float64).sum()) == float(g["checksum"])
    return verts, F, pts, g["true_sqdist"]


# ---- per-row gradient bounds (round-3 review: the surface backward is a deterministic gather, so it can be held to more than
# a tensor-wide max-norm) --------------------------------------------------------------------------------------------------
def fp64_surface_gradient(verts, faces, gt, choices, u, v, two_sided, scale=3000.0, tri_flags=0):
    """The gradient of batch_point_to_point / batch_point_to_surface (reference utils.py:393-502) with respect to the
    vertices, evaluated in FLOAT64 from the closed form, TERM BY TERM: every loss term (one per sampled point, one per gt
    point) owns a private copy of the 3 corners it depends on, autograd gives the term's corner gradients, and a scatter-add
    of them is the exact gradient `grad` [B,V,3]; the scatter-add of their absolute values is `mass` [B,V,3], the sum of
    |contributions| that meet in a row -- the scale an fp32 evaluation's round-off is proportional to, whatever cancels.
    Arg-min indices come from the oracle on the fp32 sampled points (what the HIP path reproduces bit for bit).
    Inputs are numpy arrays; returns (loss, grad, mass) as float64 numpy."""
    import torch
    import oracle
    from oracle import ref_ops
    tv, tf = torch.from_numpy(np.asarray(verts)), torch.from_numpy(np.asarray(faces)).long()
    tg = torch.from_numpy(np.asarray(gt))
    ch = torch.from_numpy(np.asarray(choices)).long()
    tu, tw = torch.from_numpy(np.asarray(u)), torch.from_numpy(np.asarray(v))
    b, nv, _ = tv.shape
    num, n_gt = ch.shape[1], tg.shape[1]
    pred32 = ref_ops.sample_points(tv, tf, ch, tu, tw)                    # fp32, bitwise what the kernel produces
    _, idx_p, _, idx_g = oracle.chamfer_nn(tg.numpy(), pred32.numpy())
    idx_p, idx_g = torch.from_numpy(idx_p).long(), torch.from_numpy(idx_g).long()
    dv, dg, du, dw = tv.double(), tg.double(), tu.double(), tw.double()

    def corners_of(face_ids):                                             # [B,N] face ids -> vertex ids [B,N,3], leaf corners [B,N,3,3]
        vid = tf[face_ids]
        c = torch.gather(dv, 1, vid.reshape(b, -1, 1).expand(-1, -1, 3)).reshape(b, -1, 3, 3)
        return vid, c.clone().requires_grad_(True)

    def sample(c, uu, ww):
        return (1 - uu)[..., None] * c[:, :, 0] + (uu * (1 - ww))[..., None] * c[:, :, 1] + (uu * ww)[..., None] * c[:, :, 2]

    groups = []
    # terms of the sampled points: |gt[nn(s)] - pred_s|^2
    vid_s, c_s = corners_of(ch)
    near = torch.gather(dg, 1, idx_g.unsqueeze(-1).expand(-1, -1, 3))
    loss = (scale / (b * num)) * ((near - sample(c_s, du, dw)) ** 2).sum()
    groups.append((vid_s, c_s))
    if two_sided:     # terms of the gt points: |pred[nn(g)] - g|^2 -- the corners of the face sample nn(g) was drawn on
        face_g = torch.gather(ch, 1, idx_p)
        vid_g, c_g = corners_of(face_g)
        ug, wg = torch.gather(du, 1, idx_p), torch.gather(dw, 1, idx_p)
        loss = loss + (scale / (b * n_gt)) * ((sample(c_g, ug, wg) - dg) ** 2).sum()
    else:             # |closest_on_triangle(g) - g|^2 for the winner of the point-to-triangle scan (its region code selects the formula)
        _, opt, tri = oracle.tri_scan_indexed(tg.numpy(), tv.numpy(), tf.numpy(), tri_flags)
        vid_g, c_g = corners_of(torch.from_numpy(tri).long())
        flat = c_g.reshape(-1, 3, 3)
        closest = ref_ops.closest_point(dg.reshape(-1, 3), flat[:, 0], flat[:, 1], flat[:, 2], torch.from_numpy(opt).reshape(-1))
        loss = loss + (scale / (b * n_gt)) * ((closest - dg.reshape(-1, 3)) ** 2).sum()
    groups.append((vid_g, c_g))
    loss.backward()
    grad = torch.zeros(b, nv, 3, dtype=torch.float64)
    mass = torch.zeros(b, nv, 3, dtype=torch.float64)
    floor = torch.zeros(b, nv, 3, dtype=torch.float64)
    # Every term is 2 * coef * (a DIFFERENCE of two fp32 coordinates) * (a weight <= 1): the difference carries the absolute
    # rounding of the coordinates themselves (ulps of max|coordinate|), however small it is -- a gt point lying 1e-5 from the
    # surface has a term a thousand times smaller than that rounding.  `floor` = one coordinate ulp through every term that
    # meets in the element; the bound is rtol * mass + floor_ulps * floor.
    ulp = float(np.finfo(np.float32).eps) * float(max(np.abs(finite_part(verts)).max(), np.abs(gt).max()))   # (finite_part: below)
    for (vid, c), coef in zip(groups, (scale / (b * num), scale / (b * n_gt))):
        index = vid.reshape(b, -1, 1).expand(-1, -1, 3)
        g = c.grad.reshape(b, -1, 3)
        grad.scatter_add_(1, index, g)
        mass.scatter_add_(1, index, g.abs())
        floor.scatter_add_(1, index, torch.full_like(g, 2.0 * coef * ulp))
    return float(loss.detach()), grad.numpy(), mass.numpy(), floor.numpy()


def rows_close(actual, exact, mass, rtol, what="", floor=None, floor_ulps=0.0):
    """|actual - exact| <= rtol * mass + floor_ulps * floor ELEMENT BY ELEMENT, where mass = the sum of the absolute
    contributions that meet in the element (and floor = one coordinate ulp through each of them, see
    fp64_surface_gradient): a wrong neighbour or a dropped term on a low-gradient vertex fails here even when the tensor's
    largest entry is 1000x bigger (the max-norm `close` of test_ops_parity_gpu.py would let it pass)."""
    actual, exact, mass = (np.asarray(x, np.float64) for x in (actual, exact, mass))
    err = np.abs(actual - exact)
    bound = rtol * mass + (0.0 if floor is None else floor_ulps * np.asarray(floor, np.float64)) + 1e-30
    worst = float((err / bound).max())
    log = os.environ.get("GEOM_MARGIN_LOG")
    if log:                       # margins of a run, for choosing / reporting the bounds (LAB_NOTES.md quotes them)
        with open(log, "a") as f:
            f.write("%s: worst element at %.3g of its bound (rtol %g, floor %g ulp), max abs err %.3g, max |exact| %.3g\n"
                    % (what, worst, rtol, floor_ulps, err.max(), np.abs(exact).max()))
    assert worst <= 1.0, "%s: worst element is %.2fx its bound (rtol %g of the row's term mass + %g coordinate ulps per term); " \
                         "max err %g" % (what, worst, rtol, floor_ulps, err.max())
    return worst


def nonfinite_close(got, want64, mass, rtol, what="", kinds=True):
    """`got` (an fp32 evaluation) against `want64` (float64) where `want64` holds NaN and Inf, in this order:
      1. isfinite(got) == isfinite(want64) for EVERY element;
      2. kinds: NaN, +Inf and -Inf agree element by element (False where only the mask is determinate: Inf - Inf in a variance);
      3. the elements finite in want64 pass rows_close(rtol) -- the bound the finite test of the same kernel uses.
    mass: the |.|-chain of the float64 run with every non-finite factor replaced by 0 (finite wherever want64 is)."""
    got, want64, mass = (np.asarray(x.detach().cpu() if hasattr(x, "detach") else x, np.float64) for x in (got, want64, mass))
    assert got.shape == want64.shape == mass.shape, "%s: shapes %s %s %s" % (what, got.shape, want64.shape, mass.shape)
    fin_got, fin_want = np.isfinite(got), np.isfinite(want64)
    bad = np.argwhere(fin_got != fin_want)
    assert not len(bad), "%s: %d elements finite on one side only (of %d non-finite in float64), first at %s: got %r, float64 %r" \
        % (what, len(bad), (~fin_want).sum(), tuple(bad[0]), got[tuple(bad[0])], want64[tuple(bad[0])])
    if kinds:
        for name, pick in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
            bad = np.argwhere(pick(got) != pick(want64))
            assert not len(bad), "%s: %s differs at %d elements, first at %s: got %r, float64 %r" \
                % (what, name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want64[tuple(bad[0])])
    if not fin_want.any():
        return 0.0
    assert np.isfinite(mass[fin_want]).all(), "%s: the mass of a finite element is not finite" % what
    return rows_close(got[fin_want], want64[fin_want], mass[fin_want], rtol, what)


def finite_part(t):
    """t with every non-finite element replaced by 0 (torch or numpy): the factor a mass chain carries in its place."""
    import torch
    if torch.is_tensor(t):
        return torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    return np.where(np.isfinite(t), t, 0.0)


# ---- the pooling's vertex-position gradient per element (oracle/ref_ops.py pool_vertex_gradient) -------------------------------
POOL_NEAR = 1e-3          # texels: vertices closer than this to a texel line are left out (the gradient jumps across the line;
#                           the fp32 texel coordinate is within 1e-5 of the float64 one: 100 times the rounding)
POOL_MAX_LEFT_OUT = 0.02  # share of a case's vertices that may be left out
POOL_ROW_RTOL = 8 * float(np.finfo(np.float32).eps)   # the project's bar for a short fp32 product chain
POOL_FLOOR_ULPS = 1.0     # texel-coordinate ulps through every term


def pool_vertex_gradient_close(got, blocks, verts, cam_mat, cam_pos, grad_out, what):
    """`got` [B,V,3] -- an fp32 evaluation of d (sum grad_out * pooled features) / d verts -- against the float64 closed form
    (ref_ops.pool_vertex_gradient, given the SAME fp32 cameras), element by element: rows_close(POOL_ROW_RTOL of the element's
    term mass + POOL_FLOOR_ULPS texel-coordinate ulps through every term) on the vertices at least POOL_NEAR from every texel
    line -- at most POOL_MAX_LEFT_OUT of the case's vertices may sit closer --, and exactly zero wherever the float64 gradient
    is exactly zero (the clamp lets nothing through).  Arguments are torch tensors (any device) or numpy arrays.  Returns
    {"keep": [B,V] bool, "zero_rows": all-zero rows of the float64 gradient, "zero_checked": those of them that are kept,
    "live_rows": kept rows with a gradient, "worst": the worst element as a share of its bound}."""
    import torch
    from oracle import ref_ops
    cpu = lambda t: torch.as_tensor(t).detach().cpu()
    grad, mass, floor, near = ref_ops.pool_vertex_gradient([cpu(m) for m in blocks], cpu(verts), cpu(cam_mat), cpu(cam_pos),
                                                           cpu(grad_out))
    keep = near >= POOL_NEAR
    assert (~keep).mean() <= POOL_MAX_LEFT_OUT, "%s: %d of %d vertices within %g of a texel line" % (what, (~keep).sum(), keep.size,
                                                                                                 POOL_NEAR)
    got = cpu(got).numpy()
    zero = keep & (grad == 0).all(-1)
    assert (got[zero] == 0).all(), "%s: a vertex the clamp holds on both axes has a gradient" % what
    live = keep & ~zero
    worst = rows_close(got[live], grad[live], mass[live], POOL_ROW_RTOL, what, floor=floor[live], floor_ulps=POOL_FLOOR_ULPS)
    return {"keep": keep, "zero_rows": int((grad == 0).all(-1).sum()), "zero_checked": int(zero.sum()), "live_rows": int(live.sum()),
            "worst": worst}


# ---- the per-vertex BatchNorm + ReLU + residual average in float64, with every output's term mass (csrc/vertex_bn.hip) ----------
BN_EPS32 = 2.0 ** -24
# the longest chain of fp32 additions in either kernel's reduction (16 values per thread, 6 shuffle steps, 4 wave partials) + the
# project's allowance of 8 for the products around it (test_layer_gradients_element_by_element_against_float64)
BN_ROW_RTOL = (16 + 6 + 4 + 8) * BN_EPS32
BN_EVAL_RTOL = 8 * BN_EPS32        # eval mode: no reduction in the forward
BN_MAX_KNIFE = 1e-3                # share of a case's elements that may sit on the ReLU's kink (a condition, not a measurement)


def vertex_bn64(x, gamma, beta, eps, relu, residual, scale, grad_out, grad_out2=None, running=None, momentum=None,
                old_running=None, rtol=None):
    """`(residual + act(BatchNorm1d(verts)(x))) * scale` on [B,V,C] and its backward in FLOAT64 on the host (numpy): one statistic
    per vertex over its n = B * C values.  Training mode (running is None) generalises bn64: batch statistics, biased variance in
    the normalisation; eval mode normalises with running = (mean, var).  gamma / beta None = 1 / 0; residual None = no residual
    (the scale is then 1); grad_out None = forward only.

    Returns (exact, mass, knife): two dicts keyed out, pre (the value the ReLU is applied to), save_mean, var, save_invstd,
    running_mean, running_var (training with old_running = (mean, var) and momentum; the variance unbiased when n > 1), grad_x,
    grad_residual, grad_weight, grad_bias -- `mass` holds what an fp32 evaluation's round-off of that output is proportional to,
    whatever cancels (helpers.rows_close): with s = 1 / sqrt(var + eps), xh = (x - mean) s, D = s |mean| (the mean's own rounding
    seen in normalised units), k = |gamma| s, gy = |grad_out + grad_out2| * scale * relu', P = mean gy, Q = mean(gy |xh|):
        out            scale (|residual| + |gamma| (|xh| + D) + |beta|)
        grad_x         k (gy + P + |xh| Q + D (Q + |xh| P))
        grad_weight    sum gy (|xh| + D)            grad_bias   sum gy
        var            var                          running_var   (1 - m) |old| + m var n / (n - 1)
        save_mean      mean |x|                     running_mean  (1 - m) |old| + m mean |x|          save_invstd   s
    knife [B,V,C] bool: the elements on the ReLU's kink -- |pre| <= 2 * rtol * (the mass of pre): an fp32 evaluation may take
    the other branch there.  They are to be left out of the forward comparison, and the gradients returned here are those of
    the upstream gradient with zeros at them (hand the kernel the same: `grad_out * ~knife`).  rtol defaults to BN_ROW_RTOL
    (BN_EVAL_RTOL in eval mode)."""
    x = np.asarray(x, np.float64)
    b, nv, c = x.shape
    n = b * c
    training = running is None
    if rtol is None:
        rtol = BN_ROW_RTOL if training else BN_EVAL_RTOL
    col = lambda t: np.asarray(t, np.float64).reshape(1, nv, 1)
    g = col(gamma) if gamma is not None else np.ones((1, nv, 1))
    be = col(beta) if beta is not None else np.zeros((1, nv, 1))
    mean_abs = np.abs(x).mean(axis=(0, 2))
    if training:
        mean = x.mean(axis=(0, 2))
        var = ((x - col(mean)) ** 2).mean(axis=(0, 2))
    else:
        mean, var = (np.asarray(t, np.float64) for t in running)
    s = 1.0 / np.sqrt(var + eps)
    xh = (x - col(mean)) * col(s)
    D = col(s * np.abs(mean))
    pre = xh * g + be
    pre_mass = np.abs(g) * (np.abs(xh) + D) + np.abs(be)
    knife = (np.abs(pre) <= 2.0 * rtol * pre_mass) if relu else np.zeros(x.shape, bool)
    act = np.maximum(pre, 0.0) if relu else pre
    exact = {"pre": pre, "save_mean": mean, "var": var, "save_invstd": s}
    mass = {"pre": pre_mass, "save_mean": mean_abs, "var": var, "save_invstd": s}
    if residual is not None:
        r = np.asarray(residual, np.float64)
        exact["out"], mass["out"] = (r + act) * scale, abs(scale) * (np.abs(r) + pre_mass)
    else:
        scale = 1.0
        exact["out"], mass["out"] = act, pre_mass
    if training and old_running is not None:
        old_mean, old_var = (np.asarray(t, np.float64) for t in old_running)
        unbiased = var * (n / (n - 1.0)) if n > 1 else var
        exact["running_mean"] = (1 - momentum) * old_mean + momentum * mean
        mass["running_mean"] = (1 - momentum) * np.abs(old_mean) + momentum * mean_abs
        exact["running_var"] = (1 - momentum) * old_var + momentum * unbiased
        mass["running_var"] = (1 - momentum) * np.abs(old_var) + momentum * unbiased
    if grad_out is not None:
        go = np.asarray(grad_out, np.float64) + (0.0 if grad_out2 is None else np.asarray(grad_out2, np.float64))
        go = go * ~knife
        exact["grad_residual"] = go * scale
        dact = ~(pre <= 0.0) if relu else np.ones(x.shape, bool)        # torch's threshold_backward: a NaN lets the gradient through
        gy = np.where(dact, go * scale, 0.0)                            # (a select, as torch's: a non-finite gradient behind a closed ReLU is 0)
        ay, axh = np.abs(gy), np.abs(xh)
        sum_g, sum_gx = gy.sum(axis=(0, 2)), (gy * xh).sum(axis=(0, 2))
        exact["grad_bias"], mass["grad_bias"] = sum_g, ay.sum(axis=(0, 2))
        exact["grad_weight"], mass["grad_weight"] = sum_gx, (ay * (axh + D)).sum(axis=(0, 2))
        exact["grad_x"] = g * col(s) * (gy - col(sum_g / n) - xh * col(sum_gx / n))
        P, Q = col(ay.mean(axis=(0, 2))), col((ay * axh).mean(axis=(0, 2)))
        mass["grad_x"] = np.abs(g) * col(s) * (ay + P + axh * Q + D * (Q + axh * P))
    return exact, mass, knife


# ---- the regularisers of one deformation stage term by term (csrc/regularizers.hip) ------------------------------------------------
def stage_regularisers_chain(prev, cur, adj_orig, faces, c_lap, c_move, c_edge, gout, absolute=False, ulps=False, aggregate=None):
    """c_edge * sum_faces(|e1|^2 + |e2|^2 + |e3|^2)(cur) + c_lap * sum |lap(prev - cur)|^2 + c_move * sum |prev - cur|^2 and its
    gradients, written out term by term in the dtype of `cur` (torch, host): {"value", "lapd" = lap(prev - cur) [B,V,3],
    "grad_prev" = gout * d value / d (prev - cur), "grad_edge" = the edge term's share of grad_cur, "grad_cur" = grad_edge -
    grad_prev}.  lap(d)[v] = d[v] - (sum_{j in row v} d[j] - d[v]) / deg[v] with the rows of the binary adjacency `adj_orig`
    (self loops included), its transpose the same with 1 / deg[j] inside the sum (ref_ops.lap_info, utils.py:654-662).
    absolute: the same chain with every matrix entry, every coordinate difference and every term replaced by its absolute
    value -- the masses of rows_close (the value is not formed).  ulps (with absolute): every coordinate difference replaced
    by one fp32 ulp of the two coordinates it is formed from, |a| + |b| -- the floor of rows_close.  aggregate: torch.matmul (the
    default: the reference's dense product, where 0 * NaN poisons every row of the mesh) or ref_ops.sparse_aggregate (the sum
    over a row's STORED entries, what the kernels walk: a non-finite row reaches its neighbours only)."""
    import torch
    one_ulp = float(np.finfo(np.float32).eps)
    A = adj_orig.to(cur.dtype)
    matmul = aggregate or torch.matmul
    inv_deg = (1.0 / (A.sum(1) - 1)).view(-1, 1)
    pv = prev if prev.dim() == 3 else prev.unsqueeze(0)

    def diff(a, b):
        if ulps:
            return one_ulp * (a.abs() + b.abs())
        return (a - b).abs() if absolute else a - b

    sign = 1.0 if absolute else -1.0
    d = diff(pv, cur)
    lapd = d + sign * (matmul(A, d) + sign * d) * inv_deg
    lt = lapd + sign * (matmul(A, lapd * inv_deg) + sign * lapd * inv_deg)
    grad_prev = (lt * (2.0 * c_lap) + d * (2.0 * c_move)) * abs(gout) if absolute else (lt * (2.0 * c_lap) + d * (2.0 * c_move)) * gout
    out = {"lapd": lapd, "grad_prev": grad_prev}
    grad_edge = torch.zeros_like(cur)
    if c_edge != 0.0 and faces.shape[0]:
        i1, i2, i3 = faces[:, 0], faces[:, 1], faces[:, 2]
        p1, p2, p3 = cur[:, i1], cur[:, i2], cur[:, i3]
        e1, e2, e3 = diff(p2, p1), diff(p3, p1), diff(p2, p3)
        grad_edge.index_add_(1, i1, (e1 + e2) * (1.0 if absolute else -1.0))
        grad_edge.index_add_(1, i2, e1 + e3)
        grad_edge.index_add_(1, i3, e2 + sign * e3)
        grad_edge = grad_edge * (2.0 * c_edge * (abs(gout) if absolute else gout))
        edge_value = c_edge * ((e1 ** 2).sum() + (e2 ** 2).sum() + (e3 ** 2).sum())
    else:
        edge_value = 0.0
    out["grad_edge"] = grad_edge
    out["grad_cur"] = grad_edge + sign * grad_prev
    if not absolute:
        out["value"] = edge_value + c_lap * (lapd ** 2).sum() + c_move * (d ** 2).sum()
    return out
