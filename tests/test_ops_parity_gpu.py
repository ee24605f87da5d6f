"""-m gpu parity of the sampling / loss / 0N-GCN stages (through the C ABI and the python
mirror of the reference interface) against (a) the fixtures the reference itself produced
and (b) the CPU restatement at the BASELINE sizes.

Tolerances: sampled points bit-exact (same three products and two sums per coordinate);
losses 1e-5 relative (north-star bar); gradients 1e-4 relative to the gradient scale
(fp32 atomics / different but equivalent summation order)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import bits, fp64_surface_gradient, golden, pool_vertex_gradient_close, rows_close, stage_regularisers_chain
from geometrics_amd import backward_pass, layers, meshgen, ops, utils
from oracle import ref_ops

pytestmark = pytest.mark.gpu


def dev(a, gpu, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t.requires_grad_(True) if grad else t


def close(actual, expected, rtol, scale=None):
    """MAX-NORM closeness: |actual - expected| <= rtol * max|expected| element-wise.  Deliberately not per-element relative:
    the gradients compared with it are sums whose fp32 terms arrive in a different order on the GPU (atomics-free gathers,
    split-K partials), so an entry 1000x smaller than the largest one legitimately carries the ABSOLUTE round-off of the
    large terms that cancelled into it -- a 10 % relative error there is noise, and would pass; what the bound does catch
    is any error that matters at the scale of the tensor (a wrong neighbour, a dropped term, a transposed tile)."""
    actual, expected = np.asarray(actual, np.float64), np.asarray(expected, np.float64)
    scale = np.abs(expected).max() if scale is None else scale
    assert np.abs(actual - expected).max() <= rtol * max(scale, 1e-30), \
        "max abs err %g vs tol %g" % (np.abs(actual - expected).max(), rtol * scale)


def draws(g, gpu):
    return dev(g["choices"], gpu), dev(g["u"], gpu), dev(g["v"], gpu)


# Per-row gradient bounds (helpers.rows_close): |error| <= rtol * (sum of the absolute contributions meeting in the element)
# + floor_ulps coordinate ulps through each of those contributions.  The sampling backward is a weighted sum of given vectors:
# a few fp32 roundings per term, no floor.  The surface-loss backward forms its terms from fp32 DIFFERENCES of coordinates
# (pred - gt, closest - gt: numbers of size ~0.5 whose difference may be 1e-5), so each term carries the coordinates' own
# rounding whatever its size (the floor: 1 ulp of max|coordinate| per term = 3e-8 here, where a single wrong or dropped
# term is 1e-4 .. 1e-2), plus the plane / edge projections of the point-to-triangle candidates (the rtol part; the
# reference's own fp32 autograd sits at 1.7e-5 of the row mass on the same inputs).
# Measured margins at these bounds (GEOM_MARGIN_LOG, MI355X): the worst element sits at 0.29 (sampling), 0.11 / 0.06 (fixtures)
# and 0.43 / 0.22 (BASELINE size, point-to-point / point-to-surface) of its bound.
ROW_RTOL_SAMPLING = 5e-7
ROW_RTOL_SURFACE = 5e-6
ROW_FLOOR_ULPS = 1.0


# ---------------------------------------------------------------- adjacency ----
def test_adjacency_built_on_the_device_matches_reference_vectors(gpu):
    """utils.adj_init / calc_adj / normalize_adj (reference utils.py:96-131) ON THE DEVICE, bit for bit against the
    matrices the imported reference produced (tests/golden adj_ico162: the full dense pair; adj_482: the reference's own
    template mesh, non-zeros) -- the CPU suite holds the same comparison for host tensors -- and the CSR / ELL tables the
    aggregation kernels read are exactly that matrix."""
    g = golden("adj_ico162")
    info = utils.adj_init(dev(g["faces"], gpu))
    assert info["adj"].is_cuda and info["adj_orig"].is_cuda and info["faces"].dtype == torch.int64
    np.testing.assert_array_equal(info["adj_orig"].cpu().numpy(), g["adj_orig"])
    np.testing.assert_array_equal(bits(info["adj"].cpu().numpy()), bits(g["adj"]))
    np.testing.assert_array_equal(bits(utils.normalize_adj(utils.calc_adj(dev(g["faces"], gpu))).cpu().numpy()), bits(g["adj"]))
    g = golden("adj_482")
    info = utils.adj_init(dev(g["faces"], gpu))
    dense = info["adj"].cpu().numpy()
    r, c = np.nonzero(dense)
    np.testing.assert_array_equal(r, g["nnz_rows"])
    np.testing.assert_array_equal(c, g["nnz_cols"])
    np.testing.assert_array_equal(bits(dense[r, c]), bits(g["nnz_vals"]))
    csr = layers.adjacency_csr(info["adj"])                       # what the kernels read: same pattern, same value bits
    rowptr, col, val = (t.cpu().numpy() for t in (csr.rowptr, csr.col, csr.val))
    assert csr.nnz == len(r) == 3362
    np.testing.assert_array_equal(np.repeat(np.arange(482), np.diff(rowptr)), r)
    np.testing.assert_array_equal(col, c)
    np.testing.assert_array_equal(bits(val), bits(g["nnz_vals"]))


# ------------------------------------------------------------------ sampling ----
def test_batch_sample_matches_reference_fixture(gpu):
    g = golden("sample_v162")
    verts = dev(g["verts"], gpu, grad=True)
    pts = utils.batch_sample(verts, dev(g["faces"], gpu), num=500, draws=draws(g, gpu))
    np.testing.assert_array_equal(bits(pts.detach().cpu().numpy()), bits(g["points"]))
    pts.backward(dev(g["grad_points"], gpu))
    close(verts.grad.cpu().numpy(), g["grad_verts"], 1e-5)
    # per ROW, against float64: grad_verts[v] = sum over the samples on v's faces of weight * grad_point, all weights >= 0, so
    # the same backward applied to |grad_points| is the mass of absolute contributions that meet in the row
    ch, u, v = (torch.from_numpy(g[k]) for k in ("choices", "u", "v"))
    v64 = torch.from_numpy(g["verts"]).double().requires_grad_(True)
    p64 = ref_ops.sample_points(v64, torch.from_numpy(g["faces"]), ch, u.double(), v.double())
    exact, = torch.autograd.grad(p64, v64, torch.from_numpy(g["grad_points"]).double(), retain_graph=True)
    mass, = torch.autograd.grad(p64, v64, torch.from_numpy(g["grad_points"]).double().abs())
    rows_close(verts.grad.cpu().numpy(), exact.numpy(), mass.numpy(), ROW_RTOL_SAMPLING, "batch_sample grad_verts")


def test_face_areas_and_random_draws(gpu):
    V, Fc = meshgen.icosphere(4)
    verts = meshgen.jittered_batch(V, 2)
    areas = ops.face_areas(dev(verts, gpu), dev(Fc, gpu))
    ref = ref_ops.face_areas(torch.from_numpy(verts), torch.from_numpy(Fc))
    np.testing.assert_allclose(areas.cpu().numpy(), ref.numpy(), rtol=1e-6)      # multinomial weights only
    torch.manual_seed(0)
    choices, u, v = ops.draw_samples(dev(verts, gpu), dev(Fc, gpu), 200000)
    assert choices.shape == (2, 200000) and int(choices.max()) < Fc.shape[0] and choices.dtype == torch.int64
    freq = torch.bincount(choices[0], minlength=Fc.shape[0]).double().cpu() / 200000
    p = (ref[0] / ref[0].sum()).double()
    assert float((freq - p).abs().max()) < 4e-4                       # area-weighted
    assert abs(float((u * u).mean()) - 0.5) < 5e-3 and abs(float(v.mean()) - 0.5) < 5e-3   # u = sqrt(U)
    pts = utils.batch_sample(dev(verts, gpu), dev(Fc, gpu), num=3000)
    assert pts.shape == (2, 3000, 3)
    r = pts.norm(dim=-1)
    assert float(r.min()) > 0.3 and float(r.max()) < 0.6               # on the jittered sphere


# -------------------------------------------------------------------- losses ----
@pytest.mark.parametrize("name,fn", [("p2p_v162", "batch_point_to_point"), ("p2s_v162", "batch_point_to_surface")])
def test_losses_match_reference_fixture(gpu, name, fn):
    g = golden(name)
    verts = dev(g["verts"], gpu, grad=True)
    info = {"faces": dev(g["faces"], gpu)}
    loss, f1 = getattr(utils, fn)(verts, info, dev(g["gt"], gpu), num=500, f1=True, draws=draws(g, gpu))
    loss.backward()
    close(loss.item(), g["loss"], 1e-5)
    assert abs(f1 - float(g["f1"])) < 1e-9
    close(verts.grad.cpu().numpy(), g["grad_verts"], 1e-4)       # vs the reference's own fp32 autograd (itself round-off noisy)
    assert isinstance(f1, float) and loss.dim() == 0
    # per ROW against the float64 closed form (helpers.fp64_surface_gradient): the backward is an atomics-free gather in a
    # fixed order, so every vertex row is held to its OWN scale, not to the tensor's largest entry
    exact_loss, exact, mass, floor = fp64_surface_gradient(g["verts"], g["faces"], g["gt"], g["choices"], g["u"], g["v"],
                                                           two_sided=(fn == "batch_point_to_point"))
    close(loss.item(), exact_loss, 1e-5)
    rows_close(verts.grad.cpu().numpy(), exact, mass, ROW_RTOL_SURFACE, fn + " grad_verts", floor, ROW_FLOOR_ULPS)


def test_calc_point_to_line_all_options(gpu):
    g = golden("p2line_options")
    a, b, c = (dev(g[k], gpu, grad=True) for k in "abc")
    loss = utils.calc_point_to_line(dev(g["p"], gpu), [a, b, c], dev(g["option"], gpu))
    loss.backward()
    close(loss.item(), g["loss"], 1e-5)
    for t, k in ((a, "grad_a"), (b, "grad_b"), (c, "grad_c")):
        close(t.grad.cpu().numpy(), g[k], 2e-4)


@pytest.mark.parametrize("fn", ["point_to_point", "point_to_surface"])
def test_losses_at_baseline_size(gpu, fn):
    V, Fc = meshgen.icosphere(4)
    B, S = 2, 3000
    verts = meshgen.jittered_batch(V, B)
    gt = meshgen.gt_cloud(B, S)
    ch, u, v = meshgen.sampling_draws(verts, Fc, S)
    cv = torch.from_numpy(verts).requires_grad_(True)
    ref = getattr(ref_ops, fn)(cv, torch.from_numpy(Fc), torch.from_numpy(gt), torch.from_numpy(ch),
                               torch.from_numpy(u), torch.from_numpy(v))
    ref.backward()
    gv = dev(verts, gpu, grad=True)
    loss = getattr(utils, "batch_" + fn)(gv, {"faces": dev(Fc, gpu)}, dev(gt, gpu), num=S,
                                         draws=(dev(ch, gpu), dev(u, gpu), dev(v, gpu)))
    loss.backward()
    close(loss.item(), ref.item(), 1e-5)
    close(gv.grad.cpu().numpy(), cv.grad.numpy(), 1e-4)
    exact_loss, exact, mass, floor = fp64_surface_gradient(verts, Fc, gt, ch, u, v, two_sided=(fn == "point_to_point"))
    close(loss.item(), exact_loss, 1e-5)
    rows_close(gv.grad.cpu().numpy(), exact, mass, ROW_RTOL_SURFACE, fn + " grad_verts at the BASELINE size", floor, ROW_FLOOR_ULPS)


def test_device_sum_is_reproducible(gpu):
    x = torch.randn(24000, device=gpu)
    a, b = ops.device_sum(x), ops.device_sum(x)
    assert torch.equal(a, b)
    close(a.item(), x.double().sum().item(), 1e-5, scale=float(x.abs().sum()))


# -------------------------------------------------------------------- layers ----
CASES = {
    "ZERON_GCN": (layers.ZERON_GCN, (24, 60), F.elu),
    "BatchZERON_GCN": (layers.BatchZERON_GCN, (24, 60), F.elu),
    "Batch_Image_ZERON_GCNGCN": (layers.Batch_Image_ZERON_GCNGCN, (33, 48), F.relu),
    "Batch_Image_ZERON_GCNGCN_out3": (layers.Batch_Image_ZERON_GCNGCN, (48, 3), lambda x: x),
    "GCNMax": (layers.GCNMax, (30, 50), F.elu),
    "BatchGCNMax": (layers.BatchGCNMax, (30, 50), F.elu),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_layers_match_reference_fixture(gpu, name):
    g = golden("layer_" + name)
    cls, dims, act = CASES[name]
    layer = cls(*dims).to(gpu)
    state = {k[len("param."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")}
    layer.load_state_dict(state)                      # reference parameter names load unchanged
    adj = dev(golden("layer_adj")["adj"], gpu)
    x = dev(g["x"], gpu, grad=True)
    out = layer(x, adj, act)
    out.backward(dev(g["grad_out"], gpu))
    close(out.detach().cpu().numpy(), g["out"], 1e-5)
    close(x.grad.cpu().numpy(), g["grad_x"], 1e-4)
    for pn, p in layer.named_parameters():
        close(p.grad.cpu().numpy(), g["grad." + pn], 1e-4)


def _layer_gradient_masses(x, adj, w, b, split, gp):
    """float64 |.|-chain of a 0N-GCN layer's backward: what every gradient element's terms add up to in absolute value --
    the scale an fp32 evaluation's round-off is proportional to whatever cancels (helpers.rows_close).  gp = |grad_out * act'|."""
    k = w.shape[-1] // split
    aw, ax, aadj = w.abs(), x.abs(), adj.abs()
    gs = torch.cat((aadj.transpose(-1, -2) @ gp[..., :k], gp[..., k:]), dim=-1)          # |A|^T on the aggregated slice
    mass_x = gs @ aw.t()
    mass_w = ax.reshape(-1, ax.shape[-1]).t() @ gs.reshape(-1, gs.shape[-1])
    mass_b = gp.reshape(-1, gp.shape[-1]).sum(0)
    return mass_x, mass_w, mass_b


@pytest.mark.parametrize("name", ["BatchZERON_GCN", "Batch_Image_ZERON_GCNGCN", "Batch_Image_ZERON_GCNGCN_out3", "ZERON_GCN"])
@pytest.mark.parametrize("mesh", ["icosphere_162", "uv_sphere_482"])
def test_layer_gradients_element_by_element_against_float64(gpu, name, mesh):
    """The max-norm bound of the fixture test above would pass a wrong low-magnitude row of an aggregation backward.  Here every
    ELEMENT of grad_x, grad_weight and grad_bias is held to (terms + 8) * 2^-24 of the sum of the absolute values of ITS OWN
    terms, against the float64 evaluation of the reference formulation (oracle.ref_ops.zero_n_layer, layers.py:34-41 /
    107-116) on the same parameters -- on an icosphere and on the 482-vertex template with its 33-entry rows (table + CSR tail).
    ReLU: outputs whose float64 pre-activation lies within round-off of zero get a zero upstream gradient (both evaluations
    then differentiate through the same branch)."""
    cls, dims, act = CASES[name]
    V, Fc = meshgen.icosphere(2) if mesh == "icosphere_162" else meshgen.uv_sphere()
    adj = utils.adj_init(dev(Fc, gpu))["adj"]
    torch.manual_seed(21)
    layer = cls(*dims).to(gpu)
    batched = name != "ZERON_GCN"
    x = torch.randn(*((3,) if batched else ()), V.shape[0], dims[0], device=gpu, requires_grad=True)
    out = layer(x, adj, act)
    wname = "weight1" if hasattr(layer, "weight1") else "weight"
    w64 = getattr(layer, wname).detach().double().cpu().reshape(dims[0], dims[1]).requires_grad_(True)
    b64 = layer.bias.detach().double().cpu().requires_grad_(True)
    x64 = x.detach().double().cpu().requires_grad_(True)
    adj64 = adj.double().cpu()
    pre = ref_ops.zero_n_layer(x64, adj64, w64, b64, layer.split, lambda t: t)
    knife = pre.detach().abs() < 1e-5 * float(pre.detach().abs().max())
    ref = act(pre)
    assert float(((out.detach().double().cpu() - ref.detach()).abs() * (~knife)).max()) <= 1e-5 * float(ref.detach().abs().max())
    gout = torch.randn(out.shape, dtype=torch.float64) * (~knife)
    out.backward(gout.float().to(gpu))
    ref.backward(gout)
    # act' in float64 (0 / 1 for ReLU, elu' = 1 or exp(pre), identity 1): the |.|-chain starts from |grad_out * act'|
    if act is F.relu:
        dact = (pre.detach() > 0).double()
    elif act is F.elu:
        dact = torch.where(pre.detach() > 0, torch.ones_like(pre.detach()), pre.detach().exp())
    else:
        dact = torch.ones_like(pre.detach())
    gp = (gout.float().double() * dact).abs()
    mass_x, mass_w, mass_b = _layer_gradient_masses(x64.detach(), adj64, w64.detach(), b64.detach(), layer.split, gp)
    rows = x64.numel() // dims[0]
    eps = 2.0 ** -24
    rows_close(x.grad.cpu().numpy(), x64.grad.numpy(), mass_x.numpy(), (dims[1] + 40 + 8) * eps, name + " grad_x on " + mesh)
    rows_close(getattr(layer, wname).grad.reshape(dims[0], dims[1]).cpu().numpy(), w64.grad.numpy(), mass_w.numpy(), (rows + 8) * eps,
               name + " grad_weight on " + mesh)
    rows_close(layer.bias.grad.cpu().numpy(), b64.grad.numpy(), mass_b.numpy(), (rows + 8) * eps, name + " grad_bias on " + mesh)


def test_config4_stack_at_baseline_size(gpu):
    """963 -> 192 -> 192 -> 192 on the 2562-vertex adjacency, fwd + bwd, vs the dense restatement."""
    V, Fc = meshgen.icosphere(4)
    info = utils.adj_init(dev(Fc, gpu))
    adj = info["adj"]
    torch.manual_seed(3041)
    stack = [layers.Batch_Image_ZERON_GCNGCN(i, o).to(gpu) for i, o in ((963, 192), (192, 192), (192, 192))]
    x = torch.randn(2, V.shape[0], 963, device=gpu, requires_grad=True)
    h = x
    for l in stack:
        h = l(h, adj, F.elu)          # smooth: a ReLU mask flips on fp32-vs-fp64 knife edges at this size
    gout = torch.randn_like(h)
    h.backward(gout)
    xc = x.detach().cpu().double().requires_grad_(True)
    adj_c = adj.cpu().double()
    hc = xc
    params = []
    for l in stack:
        w = l.weight1.detach().cpu().double().requires_grad_(True)
        b = l.bias.detach().cpu().double().requires_grad_(True)
        params.append((w, b))
        hc = ref_ops.zero_n_layer(hc, adj_c, w, b, 3, F.elu)
    hc.backward(gout.cpu().double())
    close(h.detach().cpu().numpy(), hc.detach().numpy(), 1e-5)
    close(x.grad.cpu().numpy(), xc.grad.numpy(), 1e-4)
    for l, (w, b) in zip(stack, params):
        close(l.weight1.grad.cpu().numpy(), w.grad.numpy(), 1e-4)
        close(l.bias.grad.cpu().numpy(), b.grad.numpy(), 1e-4)
    csr = layers.adjacency_csr(adj)
    assert csr.nnz == 17922 and layers.adjacency_csr(adj) is csr          # V + 2E, cached


def test_relu_sign_mask_path_at_the_bench_configuration(gpu):
    """The exact kernel configuration bench.py runs -- Batch_Image_ZERON_GCNGCN with F.relu at B=8, V=2562, C=192,
    k=64: ELL forward that also stores the sign mask, backward that takes relu' from the mask -- against the float64
    dense restatement (oracle.ref_ops.zero_n_layer, reference layers.py:107-116).  ReLU is not continuous in its
    derivative: output elements whose float64 pre-activation lies within round-off of zero are left out of the forward
    comparison and get a zero upstream gradient, so both sides differentiate through the same branch."""
    V, Fc = meshgen.icosphere(4)
    adj = utils.adj_init(dev(Fc, gpu))["adj"]
    torch.manual_seed(77)
    for cin in (963, 192):
        layer = layers.Batch_Image_ZERON_GCNGCN(cin, 192).to(gpu)
        x = torch.randn(8, V.shape[0], cin, device=gpu, requires_grad=True)
        out = layer(x, adj, F.relu)
        xc = x.detach().cpu().double().requires_grad_(True)
        w = layer.weight1.detach().cpu().double().requires_grad_(True)
        b = layer.bias.detach().cpu().double().requires_grad_(True)
        pre = ref_ops.zero_n_layer(xc, adj.cpu().double(), w, b, 3, lambda t: t)
        knife = pre.detach().abs() < 1e-5 * float(pre.detach().abs().max())
        assert 0 < int(knife.sum()) < 1e-3 * knife.numel()
        ref = torch.relu(pre)
        o = out.detach().cpu().double()
        assert float(((o - ref.detach()).abs() * (~knife)).max()) <= 1e-5 * float(ref.detach().abs().max())
        gout = torch.randn(out.shape, dtype=torch.float64) * (~knife)
        out.backward(gout.float().to(gpu))
        ref.backward(gout)
        close(x.grad.cpu().numpy(), xc.grad.numpy(), 1e-4)
        close(layer.weight1.grad.cpu().numpy(), w.grad.numpy(), 1e-4)
        close(layer.bias.grad.cpu().numpy(), b.grad.numpy(), 1e-4)


@pytest.mark.parametrize("mesh", ["482.obj", "uv_sphere"])
@pytest.mark.parametrize("act", [F.relu, F.elu])
def test_long_rows_take_the_ell_kernel_with_a_csr_tail(gpu, mesh, act):
    """The reference's own training template (GEOMetrics.py:44: 482.obj, two poles with 32 neighbours -> rows of 33
    entries next to rows of 5-9) must run on the fast table kernel: table width 8 + a CSR tail for the few longer rows.
    Checked against the generic CSR kernel (same summation order -> same bits) and the float64 dense restatement."""
    from geometrics_amd import _lib as L
    if mesh == "482.obj":
        faces = dev(golden("adj_482")["faces"], gpu)
    else:
        faces = dev(meshgen.uv_sphere()[1], gpu)
    adj = utils.adj_init(faces)["adj"]
    csr = layers.adjacency_csr(adj)
    assert csr.ell_w == 8 and csr.over is not None and csr.over_t is not None
    lens = (csr.rowptr[1:] - csr.rowptr[:-1])
    assert int(lens.max()) == 33 and int(csr.over[0][-1]) == int((lens - 8).clamp_min(0).sum())
    B, nv, C, k = 4, 482, 192, 64
    torch.manual_seed(9)
    layer = layers.Batch_Image_ZERON_GCNGCN(40, C).to(gpu)
    x = torch.randn(B, nv, 40, device=gpu, requires_grad=True)
    out = layer(x, adj, act)
    gout = torch.randn_like(out)
    out.backward(gout)
    # generic CSR kernel on the same support: identical bits (same neighbour order)
    sup = torch.matmul(x.detach(), layer.weight1.detach().squeeze(0))
    ref = torch.empty_like(sup)
    code = 1 if act is F.relu else 2
    L.call("geom_zn_gcn_aggregate_fwd_f32", B, nv, C, k, csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(),
           sup.data_ptr(), layer.bias.data_ptr(), code, ref.data_ptr())
    assert torch.equal(out.detach(), ref)
    gs_ref, gb_ref = torch.empty_like(sup), torch.empty(C, device=gpu)
    scr = torch.empty(L.lib().geom_zn_gcn_bwd_scratch_floats(B, nv, C), device=gpu)
    L.call("geom_zn_gcn_aggregate_bwd_f32", B, nv, C, k, csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(), csr.val_t.data_ptr(),
           gout.data_ptr(), ref.data_ptr(), code, gs_ref.data_ptr(), gb_ref.data_ptr(), scr.data_ptr())
    close(layer.bias.grad.cpu().numpy(), gb_ref.cpu().numpy(), 1e-5)
    gx_ref = torch.matmul(gs_ref, layer.weight1.detach().squeeze(0).t())
    close(x.grad.cpu().numpy(), gx_ref.cpu().numpy(), 1e-5)
    # float64 dense restatement (reference layers.py:107-116), smooth activation only (no knife edges)
    if act is F.elu:
        xc = x.detach().cpu().double().requires_grad_(True)
        w = layer.weight1.detach().cpu().double().requires_grad_(True)
        bb = layer.bias.detach().cpu().double().requires_grad_(True)
        oc = ref_ops.zero_n_layer(xc, adj.cpu().double(), w, bb, 3, F.elu)
        oc.backward(gout.cpu().double())
        close(out.detach().cpu().numpy(), oc.detach().numpy(), 1e-5)
        close(x.grad.cpu().numpy(), xc.grad.numpy(), 1e-4)
        close(layer.weight1.grad.cpu().numpy(), w.grad.numpy(), 1e-4)


def test_vertex_bn_eval_mode_gradients_and_batched_adjacency(gpu):
    """Two call patterns nn.BatchNorm1d / torch.matmul accept and the fused kernels do not cover natively: gradients
    through an eval()'d block (frozen-BN fine-tuning) and a per-mesh [B,V,V] adjacency; both take the library route and
    must match the plain torch formulation."""
    from geometrics_amd import models
    V, Fc = meshgen.icosphere(2)
    nv = V.shape[0]
    adj = utils.adj_init(dev(Fc, gpu))["adj"]
    torch.manual_seed(2)
    bn = models.VertexBatchNorm(nv).to(gpu)
    ref = torch.nn.BatchNorm1d(nv).to(gpu)
    x = torch.randn(3, nv, 16, device=gpu)
    bn.train(), ref.train()
    for _ in range(2):                                  # running statistics from the fused training kernel
        bn(x * 1.5 + 0.3), ref(x * 1.5 + 0.3)
    bn.eval(), ref.eval()
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = bn(xa, relu=True), torch.relu(ref(xb))
    g = torch.randn_like(ya)
    ya.backward(g), yb.backward(g)
    close(ya.detach().cpu().numpy(), yb.detach().cpu().numpy(), 1e-5)
    close(xa.grad.cpu().numpy(), xb.grad.cpu().numpy(), 1e-5)
    assert int(bn.state_dict()["num_batches_tracked"]) == 2
    big = models.VertexBatchNorm(nv).to(gpu).train()    # outside the register-resident kernel: batches are still counted
    big(torch.randn(40, nv, 192, device=gpu))
    assert int(big.state_dict()["num_batches_tracked"]) == 1
    layer = layers.BatchZERON_GCN(16, 40).to(gpu)
    out = layer(x, adj.unsqueeze(0).expand(3, nv, nv).contiguous(), F.elu)
    close(out.detach().cpu().numpy(), layer(x, adj, F.elu).detach().cpu().numpy(), 1e-5)


def test_gcn_rows_of_degree_32(gpu):
    g = golden("adj_482")
    adj = utils.adj_init(dev(g["faces"], gpu))["adj"]
    layer = layers.BatchZERON_GCN(16, 40).to(gpu)
    x = torch.randn(3, 482, 16, device=gpu)
    out = layer(x, adj, lambda t: t)
    ref = ref_ops.zero_n_layer(x.cpu().double(), adj.cpu().double(), layer.weight.detach().cpu().double(),
                               layer.bias.detach().cpu().double(), 10, lambda t: t)
    close(out.detach().cpu().numpy(), ref.numpy(), 1e-5)


def test_fused_adam_matches_torch_adam(gpu):
    from geometrics_amd import optim
    torch.manual_seed(5)
    shapes = [(1, 963, 192), (192,), (192, 192), (3,)]
    ours = [torch.randn(*s, device=gpu).requires_grad_(True) for s in shapes]
    ref = [p.detach().clone().requires_grad_(True) for p in ours]
    opt = optim.FusedAdam(ours, lr=1e-3)
    ropt = torch.optim.Adam(ref, lr=1e-3)
    for step in range(5):
        grads = [torch.randn(*s, device=gpu) for s in shapes]
        for p, r, g in zip(ours, ref, grads):
            p.grad, r.grad = g.clone(), g.clone()
        opt.step()
        ropt.step()
        for p, r in zip(ours, ref):
            close(p.detach().cpu().numpy(), r.detach().cpu().numpy(), 2e-6)
    assert float(opt.state[0]) == 5.0
    # grads supplied explicitly with a scale (the all-reduced bucket path)
    g2 = [torch.randn(*s, device=gpu) for s in shapes]
    for r, g in zip(ref, g2):
        r.grad = g / 4
    opt.step([g.clone() for g in g2], grad_scale=0.25)
    ropt.step()
    for p, r in zip(ours, ref):
        close(p.detach().cpu().numpy(), r.detach().cpu().numpy(), 2e-6)


def test_in_backward_step_protocol_cannot_step_twice_or_swallow_a_later_step(gpu):
    """Round-3 advice on FusedAdam.in_backward(): after a pass that applied the step, step(grads=...) / step(grad_scale != 1)
    must raise instead of stepping a second time; a flag nobody consumed is cleared by the next zero_grad() so that it cannot
    swallow a later, unrelated step(); and the context refuses to be entered under a multi-rank process group (checked in
    tests/test_dist_gloo.py)."""
    from geometrics_amd import optim
    p = torch.nn.Parameter(torch.ones(8, device=gpu))
    opt = optim.FusedAdam([p], lr=1e-2)
    opt._stepped_in_backward = True                    # what the end-of-pass launch leaves behind
    with pytest.raises(RuntimeError, match="stepped twice"):
        opt.step([torch.ones(8, device=gpu)])
    opt._stepped_in_backward = True
    with pytest.raises(RuntimeError, match="stepped twice"):
        opt.step(grad_scale=0.5)
    opt._stepped_in_backward = True
    opt.step()                                         # the plain call consumes the flag: a no-op
    assert opt.step_count == 0 and not opt._stepped_in_backward
    opt._stepped_in_backward = True                    # ... never consumed ...
    opt.zero_grad()                                    # ... the next iteration starts
    p.grad = torch.ones(8, device=gpu)
    opt.step()
    assert opt.step_count == 1 and float(p.detach().max()) < 1.0


def test_fused_adam_many_tensors_and_graph_replay(gpu):
    """More than 64 tensors (a deformation block has 56, GEOMetrics.py:73 hands Adam hundreds): chunks of 64 share the
    bias corrections of ONE step (only the last chunk advances the device-side state), odd sizes take the scalar tail,
    and a captured step replays with the state advancing on the device."""
    from geometrics_amd import _lib, optim
    torch.manual_seed(6)
    shapes = [(1, 1155, 192), (192,)] + [(192, 192), (192,)] * 12 + [(192, 3), (3,)] + [(7, 5), (1,), (1023,), (1025,)] * 10
    assert len(shapes) > _lib.ADAM_MAX_TENSORS
    ours = [torch.randn(*s, device=gpu).requires_grad_(True) for s in shapes]
    ref = [p.detach().clone().requires_grad_(True) for p in ours]
    opt = optim.FusedAdam(ours, lr=1e-3)
    ropt = torch.optim.Adam(ref, lr=1e-3)
    grads = [torch.randn(*s, device=gpu) for s in shapes]
    for p, r, g in zip(ours, ref, grads):
        p.grad, r.grad = g.clone(), g.clone()
    for step in range(3):
        opt.step()
        ropt.step()
    assert opt.step_count == 3
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
        ropt.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()                        # recorded, not executed
    for _ in range(4):
        graph.replay()
        ropt.step()
    torch.cuda.synchronize()
    assert opt.step_count == 8
    assert int(opt.state.view(torch.int32)[3:].abs().sum()) == 0      # arrival counters re-armed
    for p, r in zip(ours, ref):
        close(p.detach().cpu().numpy(), r.detach().cpu().numpy(), 5e-6)


def test_surface_loss_is_graph_capturable_and_stream_safe(gpu):
    """The fused loss forks a second stream; replaying it from a HIP graph must give the eager value."""
    g = golden("p2s_v162")
    verts = dev(g["verts"], gpu, grad=True)
    info = {"faces": dev(g["faces"], gpu)}
    gt, dr = dev(g["gt"], gpu), draws(g, gpu)
    for _ in range(2):
        utils.batch_point_to_surface(verts, info, gt, num=500, draws=dr).backward()
    torch.cuda.synchronize()
    verts.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = utils.batch_point_to_surface(verts, info, gt, num=500, draws=dr)
        loss.backward()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    close(loss.item(), g["loss"], 1e-5)
    close(verts.grad.cpu().numpy(), g["grad_verts"], 1e-4)


def test_regularisers_match_reference_fixture(gpu):
    """Laplacian coordinates and mean squared edge length, forward + backward."""
    g = golden("regularisers_v162")
    info = utils.adj_init(dev(g["faces"], gpu))
    verts = dev(g["verts"], gpu, grad=True)
    lap = utils.batch_get_lap_info(verts, info)
    close(lap.detach().cpu().numpy(), g["lap"], 1e-5)
    lap.backward(dev(g["grad_lap"], gpu))
    close(verts.grad.cpu().numpy(), g["grad_verts_lap"], 1e-5)
    v2 = dev(g["verts"], gpu, grad=True)
    edge = utils.batch_calc_edge(v2, info)
    edge.backward()
    close(edge.item(), g["edge"], 1e-5)
    close(v2.grad.cpu().numpy(), g["grad_verts_edge"], 1e-4)


@pytest.mark.parametrize("mesh", ["uv_sphere_482", "icosphere_162"])
@pytest.mark.parametrize("template_prev", [False, True])
def test_stage_regularisers_against_the_drivers_expressions(gpu, mesh, template_prev):
    """utils.stage_regularisers (one launch per direction) against the expressions the reference's driver builds per
    deformation stage (GEOMetrics.py:147-161) from batch_calc_edge / batch_get_lap_info (utils.py:636-662), evaluated in
    FLOAT64 on the host through the oracle's restatements: the value (1e-6) and the gradients with respect to both position
    tensors (1e-5 of scale); on the 482-vertex template (two 33-entry adjacency rows, faces of very different sizes) and an
    icosphere; prev = another batch of positions (stages 2, 3) or the [V,3] template (stage 1)."""
    V, Fc = meshgen.uv_sphere() if mesh == "uv_sphere_482" else meshgen.icosphere(2)
    faces = torch.from_numpy(Fc).to(gpu)
    info = utils.adj_init(faces)
    nv, b = V.shape[0], 5
    torch.manual_seed(13)
    base = torch.from_numpy(V).to(gpu)
    cur = (base.unsqueeze(0) + 0.05 * torch.randn(b, nv, 3, device=gpu)).requires_grad_(True)
    prev = base if template_prev else (base.unsqueeze(0) + 0.05 * torch.randn(b, nv, 3, device=gpu)).requires_grad_(True)
    w_lap, w_move, w_edge = 300.0, 20.0, 300.0
    loss = utils.stage_regularisers(prev, cur, info, lap_weight=w_lap, move_weight=w_move, edge_weight=w_edge)
    loss.backward()
    adj_orig = info["adj_orig"].double().cpu()
    c64 = cur.detach().double().cpu().requires_grad_(True)
    p64 = prev.detach().double().cpu().requires_grad_(not template_prev)
    lap = lambda x: ref_ops.lap_info(x, adj_orig)
    ref = (w_edge * ref_ops.calc_edge(c64, faces.cpu()) + w_lap * torch.mean(torch.sum((lap(p64) - lap(c64)) ** 2, 2 if not template_prev else -1))
           + w_move * torch.mean(torch.sum((p64 - c64) ** 2, -1)))
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item()), (loss.item(), ref.item())
    close(cur.grad.cpu().numpy(), c64.grad.numpy(), 1e-5)
    if not template_prev:
        close(prev.grad.cpu().numpy(), p64.grad.numpy(), 1e-5)
    # ... and the composition of the separate operators on the device gives the same number
    eager = (utils.batch_calc_edge(cur.detach(), info) * w_edge
             + torch.mean(torch.sum((utils.batch_get_lap_info(prev.detach(), info) - utils.batch_get_lap_info(cur.detach(), info)) ** 2, -1)) * w_lap
             + torch.mean(torch.sum((prev.detach() - cur.detach()) ** 2, -1)) * w_move)
    assert abs(loss.item() - eager.item()) <= 1e-5 * abs(eager.item())
    # the weighted surface loss is the loss times its weight
    gt = torch.from_numpy(np.ascontiguousarray(meshgen.gt_cloud(b, 500, first=3))).to(gpu)
    ch, u, v = ops.draw_samples(cur.detach(), faces, 400)
    a = utils.batch_point_to_surface(cur.detach(), info, gt, num=400, draws=(ch, u, v))
    w = utils.batch_point_to_surface(cur.detach(), info, gt, num=400, draws=(ch, u, v), weight=0.2)
    assert abs(w.item() - 0.2 * a.item()) <= 1e-6 * abs(a.item())


STAGE_REG_CASES = ("template_482_b1", "faces_outnumber_lanes", "ico42_faces_cut", "ico162_b3_no_edge", "ico162_b3_template_prev",
                   "ico42_vertex_without_faces")


def stage_regulariser_case(name):
    """Host tensors of a case of the per-element stage-regulariser tests: (prev, cur, faces the kernels are given, the binary
    adjacency, (w_lap, w_move, w_edge)).
      template_482_b1          482 vertices, one mesh: 3856 lanes, the last workgroup part vertices and part idle
      faces_outnumber_lanes    6 vertices, 60 faces drawn from them with repetition (nf > 8 nv: the faces set the forward grid and
                               the vertex lanes run out first), the adjacency built from those faces
      ico42_faces_cut          icosphere(1) with its last 3 faces taken out of `faces` only: corner lists shorter than their rows
      ico162_b3_no_edge        three meshes, edge weight 0: the vertex -> corner tables are null
      ico162_b3_template_prev  three meshes, the [V,3] template as prev
      ico42_vertex_without_faces   icosphere(1) with every face of vertex 0 and all but one face of its last vertex taken out of
                               `faces` only: an empty corner list and a list of one"""
    rng = np.random.default_rng([545, STAGE_REG_CASES.index(name)])
    weights = (300.0, 20.0, 0.0 if name == "ico162_b3_no_edge" else 300.0)
    b = 3 if name.startswith("ico162") else 1
    if name == "faces_outnumber_lanes":
        V = rng.uniform(-0.5, 0.5, (6, 3)).astype(np.float32)
        Fc = np.stack([rng.permutation(6)[:3] for _ in range(60)]).astype(np.int64)
        assert Fc.max() == 5 and Fc.shape[0] > 8 * V.shape[0]
    else:
        V, Fc = meshgen.uv_sphere() if name == "template_482_b1" else meshgen.icosphere(2 if name.startswith("ico162") else 1)
    adj_orig = utils.calc_adj(torch.from_numpy(np.ascontiguousarray(Fc, dtype=np.int64)))
    if name == "ico42_faces_cut":
        Fc = Fc[:-3]
    elif name == "ico42_vertex_without_faces":
        last = np.flatnonzero((Fc == Fc.max()).any(1))
        assert not (Fc[last] == 0).any()
        Fc = np.delete(Fc, last[1:], axis=0)
        Fc = Fc[(Fc != 0).all(1)]
    base = torch.from_numpy(np.ascontiguousarray(V, dtype=np.float32))
    noise = lambda: torch.from_numpy((0.05 * rng.standard_normal((b,) + tuple(base.shape))).astype(np.float32))
    cur = base.unsqueeze(0) + noise()
    prev = base if name == "ico162_b3_template_prev" else base.unsqueeze(0) + noise()
    return prev, cur, torch.from_numpy(np.ascontiguousarray(Fc, dtype=np.int64)), adj_orig, weights


def stage_regulariser_bounds(prev, cur, faces, adj_orig, weights, gout):
    """float64 values, masses and floors of a case (helpers.stage_regularisers_chain; the chain itself is held to the oracle's
    restatements ref_ops.lap_info / ref_ops.calc_edge under autograd), the coefficients and rtol = (row_terms + 8) * 2^-24,
    row_terms = the longest adjacency row or corner list of the mesh."""
    b, nv, nf = cur.shape[0], cur.shape[1], faces.shape[0]
    coef = (weights[0] / (b * nv), weights[1] / (b * nv), weights[2] / (3.0 * b * nf) if nf else 0.0)
    p64, c64, a64 = prev.double(), cur.double(), adj_orig.double()
    exact = stage_regularisers_chain(p64, c64, a64, faces, *coef, gout)
    mass = stage_regularisers_chain(p64, c64, a64, faces, *coef, gout, absolute=True)
    floor = stage_regularisers_chain(p64, c64, a64, faces, *coef, gout, absolute=True, ulps=True)
    pa, ca = p64.clone().requires_grad_(True), c64.clone().requires_grad_(True)
    ref = (weights[2] * ref_ops.calc_edge(ca, faces) + weights[0] * torch.mean(torch.sum((ref_ops.lap_info(pa, a64) - ref_ops.lap_info(ca, a64)) ** 2, -1))
           + weights[1] * torch.mean(torch.sum((pa - ca) ** 2, -1)))
    (ref * gout).backward()
    scale = float(ca.grad.abs().max())
    ref = ref.detach()
    assert abs(float(ref) - float(exact["value"])) <= 1e-12 * abs(float(ref))
    assert float((ca.grad - exact["grad_cur"]).abs().max()) <= 1e-12 * scale
    if prev.dim() == 3:
        assert float((pa.grad - exact["grad_prev"]).abs().max()) <= 1e-12 * scale
    assert float((ref_ops.lap_info(p64 - c64, a64) - exact["lapd"]).abs().max()) <= 1e-12
    corners = np.bincount(faces.reshape(-1).numpy(), minlength=nv)
    row_terms = max(int(adj_orig.sum(1).max()), int(corners.max()))
    return exact, mass, floor, coef, (row_terms + 8) * 2.0 ** -24, corners


def stage_regulariser_outputs_close(got, exact, mass, floor, rtol, what, worst_allowed=1.0):
    """lapd, grad_cur and (when present) grad_prev of `got` within rtol * mass + 1 ulp-floor, element by element."""
    for key in ("lapd", "grad_cur", "grad_prev"):
        if key in got:
            worst = rows_close(got[key], exact[key].numpy(), mass[key].numpy(), rtol, "stage regularisers %s %s" % (what, key),
                               floor[key].numpy(), ROW_FLOOR_ULPS)
            assert worst <= worst_allowed, (what, key, worst)


@pytest.mark.parametrize("case", STAGE_REG_CASES)
def test_stage_regularisers_element_by_element_against_float64(gpu, case):
    """The max-norm 1e-5 of the test above passes a wrong low-gradient vertex.  Here every element of grad_cur, grad_prev and the
    saved lap(prev - cur) is held to (row_terms + 8) * 2^-24 of the sum of the absolute values of ITS OWN terms + one coordinate
    ulp through each of them (the kernel forms prev - cur and the edge vectors as fp32 differences of coordinates), the value to
    1e-6 -- at the launch shapes no other test has (stage_regulariser_case).  The same chain in fp32 torch on the host stays
    under half of the bounds: no term is missing from the masses."""
    prev, cur, faces, adj_orig, weights = stage_regulariser_case(case)
    gout = 0.7
    exact, mass, floor, coef, rtol, corners = stage_regulariser_bounds(prev, cur, faces, adj_orig, weights, gout)
    b, nv, nf = cur.shape[0], cur.shape[1], faces.shape[0]
    if case == "template_482_b1":
        assert (8 * nv) % 256 != 0 and 8 * nv > nf
    elif case == "faces_outnumber_lanes":
        assert nf > 8 * nv
    elif case == "ico42_faces_cut":
        assert (corners < adj_orig.sum(1).numpy() - 1).any() and corners.min() >= 1
    elif case == "ico42_vertex_without_faces":
        assert corners[0] == 0 and corners[-1] == 1
    host = stage_regularisers_chain(prev, cur, adj_orig, faces, *coef, gout)
    keys = ("lapd", "grad_cur") + (("grad_prev",) if prev.dim() == 3 else ())
    stage_regulariser_outputs_close({k: host[k].numpy() for k in keys}, exact, mass, floor, rtol, case + " (fp32 on the host)", 0.5)
    assert abs(float(host["value"]) - float(exact["value"])) <= 1e-6 * abs(float(exact["value"]))
    csr = layers.adjacency_csr(adj_orig.to(gpu))
    assert int((csr.rowptr[1:] - csr.rowptr[:-1]).max()) == int(adj_orig.sum(1).max())
    p_d, c_d = prev.to(gpu).requires_grad_(prev.dim() == 3), cur.to(gpu).requires_grad_(True)
    loss = ops.StageRegularisers.apply(p_d, c_d, faces.to(gpu), csr.rowptr, csr.col, csr.inv_deg, *weights)
    lapd = loss.grad_fn.saved_tensors[6]
    assert lapd.shape == cur.shape
    (loss * gout).backward()
    assert abs(loss.item() - float(exact["value"])) <= 1e-6 * abs(float(exact["value"])), (loss.item(), float(exact["value"]))
    got = {"lapd": lapd.cpu().numpy(), "grad_cur": c_d.grad.cpu().numpy()}
    if prev.dim() == 3:
        got["grad_prev"] = p_d.grad.cpu().numpy()
    stage_regulariser_outputs_close(got, exact, mass, floor, rtol, case)


@pytest.mark.parametrize("case", STAGE_REG_CASES[:2])
def test_laplacian_and_edge_operators_element_by_element_against_float64(gpu, case):
    """ops.Laplacian (both directions) and ops.EdgeSqLenSum on the 482-vertex template at one mesh and on the mesh whose faces
    outnumber its vertex lanes, against the same float64 chain and masses.  The edge backward adds with float atomics: held
    to the same mass, its bits are not."""
    prev, cur, faces, adj_orig, _ = stage_regulariser_case(case)
    a64 = adj_orig.double()
    csr = layers.adjacency_csr(adj_orig.to(gpu))
    nv = cur.shape[1]
    rtol = (max(int(adj_orig.sum(1).max()), int(np.bincount(faces.reshape(-1).numpy(), minlength=nv).max())) + 8) * 2.0 ** -24
    # both directions of lap against ref_ops.lap_info (the backward under autograd); the masses: the same sums of absolute values
    inv_deg = (1.0 / (a64.sum(1) - 1)).view(-1, 1)
    x = cur.to(gpu).requires_grad_(True)
    lap = ops.Laplacian.apply(x, csr.rowptr, csr.col, csr.inv_deg)
    g = torch.from_numpy(np.random.default_rng(586).standard_normal(tuple(cur.shape)).astype(np.float32))
    lap.backward(g.to(gpu))
    x64, g64 = cur.double(), g.double()
    assert float((ref_ops.lap_info(x64, a64) - (x64 - (a64 @ x64 - x64) * inv_deg)).abs().max()) <= 1e-12
    rows_close(lap.detach().cpu().numpy(), ref_ops.lap_info(x64, a64).numpy(), (x64.abs() + (a64 @ x64.abs() + x64.abs()) * inv_deg).numpy(),
               rtol, "Laplacian forward " + case)
    xa = x64.clone().requires_grad_(True)
    ref_ops.lap_info(xa, a64).backward(g64)
    rows_close(x.grad.cpu().numpy(), xa.grad.numpy(), (g64.abs() + a64 @ (g64.abs() * inv_deg) + g64.abs() * inv_deg).numpy(),
               rtol, "Laplacian backward " + case)
    # sum over faces of the three squared edge lengths, times an upstream gradient
    up = 0.3
    v = cur.to(gpu).requires_grad_(True)
    total = ops.EdgeSqLenSum.apply(v, faces.to(gpu))
    (total * up).backward()
    zero = torch.zeros_like(cur).double()
    exact = stage_regularisers_chain(zero, cur.double(), a64, faces, 0.0, 0.0, 1.0, up)
    mass = stage_regularisers_chain(zero, cur.double(), a64, faces, 0.0, 0.0, 1.0, up, absolute=True)
    floor = stage_regularisers_chain(zero, cur.double(), a64, faces, 0.0, 0.0, 1.0, up, absolute=True, ulps=True)
    va = cur.double().requires_grad_(True)
    ref = ref_ops.calc_edge(va, faces) * (3.0 * cur.shape[0] * faces.shape[0])
    (ref * up).backward()
    ref = ref.detach()
    assert float((va.grad - exact["grad_edge"]).abs().max()) <= 1e-12 * float(va.grad.abs().max())
    assert abs(total.item() - float(ref)) <= 1e-6 * abs(float(ref)), (total.item(), float(ref))
    rows_close(v.grad.cpu().numpy(), exact["grad_edge"].numpy(), mass["grad_edge"].numpy(), rtol, "EdgeSqLenSum backward " + case,
               floor["grad_edge"].numpy(), ROW_FLOOR_ULPS)


def test_laplacian_on_the_reference_template_mesh(gpu):
    """482.obj has two degree-32 poles: long CSR rows, and the dense product as the checker."""
    g = golden("adj_482")
    info = utils.adj_init(dev(g["faces"], gpu))
    pos = torch.randn(2, 482, 3, device=gpu, dtype=torch.float32)
    lap = utils.batch_get_lap_info(pos, info)
    orig = info["adj_orig"].double()
    p = pos.double()
    ref = p - (torch.matmul(orig, p) - p) * (1.0 / (orig.sum(1) - 1)).view(-1, 1)
    close(lap.cpu().numpy(), ref.cpu().numpy(), 1e-5)


def test_csr_cache_follows_tensor_identity_not_addresses(gpu):
    """A freed adjacency's memory is reused by the next one of the same size; the cache must not
    serve the old graph (auto_encoder.py builds one adjacency per mesh), and in-place edits must
    invalidate too."""
    g = golden("adj_ico162")
    faces = dev(g["faces"], gpu)
    layer = layers.BatchZERON_GCN(8, 40).to(gpu)
    x = torch.randn(2, 162, 8, device=gpu)

    def expect(adj):
        return ref_ops.zero_n_layer(x.cpu().double(), adj.cpu().double(), layer.weight.detach().cpu().double(),
                                    layer.bias.detach().cpu().double(), 10, lambda t: t).numpy()

    adj = utils.adj_init(faces)["adj"]
    ptr = adj.data_ptr()
    close(layer(x, adj, lambda t: t).detach().cpu().numpy(), expect(adj), 1e-5)
    ring = torch.roll(torch.eye(162, device=gpu), 1, 1) * 0.5 + torch.eye(162, device=gpu) * 0.5
    del adj
    adj2 = torch.empty(162, 162, device=gpu)            # typically lands on the freed block
    adj2.copy_(ring)
    reused = adj2.data_ptr() == ptr
    close(layer(x, adj2, lambda t: t).detach().cpu().numpy(), expect(adj2), 1e-5)
    adj2.mul_(0.5)                                       # in-place edit bumps the version
    close(layer(x, adj2, lambda t: t).detach().cpu().numpy(), expect(adj2), 1e-5)
    assert len(layers._csr_cache) <= 4 or reused is not None


def test_deformation_block_matches_reference_fixture(gpu):
    """the 14-layer block (0N-GCN + per-vertex BatchNorm + ReLU + residual average)
    against the reference's own models.BatchMeshDeformationBlock: outputs, input/parameter gradients and the
    BatchNorm running statistics after one training-mode step; the reference state_dict loads by name."""
    from geometrics_amd import models
    g = golden("deformation_block_v162")
    block = models.BatchMeshDeformationBlock(32, 162, hidden=24, output_features=3).to(gpu)
    state = {k[len("state."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("state.")}
    missing = block.load_state_dict(state, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    block.train()
    adj = dev(g["adj"], gpu)
    feats, pooled = dev(g["features"], gpu, grad=True), dev(g["pooled"], gpu, grad=True)
    out_f, coords = block(feats, pooled, adj)
    close(out_f.detach().cpu().numpy(), g["out_features"], 2e-5)
    close(coords.detach().cpu().numpy(), g["coords"], 2e-5)
    ((out_f * dev(g["g_features"], gpu)).sum() + (coords * dev(g["g_coords"], gpu)).sum()).backward()
    close(feats.grad.cpu().numpy(), g["grad_features"], 2e-4)
    close(pooled.grad.cpu().numpy(), g["grad_pooled"], 2e-4)
    params = dict(block.named_parameters())
    for k in [k[len("grad."):] for k in g if k.startswith("grad.") and k not in ("grad.features", "grad.pooled")]:
        close(params[k].grad.cpu().numpy(), g["grad." + k], 3e-4)
    saved = block.state_dict()
    for k in [k[len("after."):] for k in g if k.startswith("after.")]:
        close(saved[k].cpu().numpy(), g["after." + k], 1e-5)
    assert int(saved["bn1.num_batches_tracked"]) == 1 and int(saved["bn14.num_batches_tracked"]) == 0
    # eval mode uses the running statistics (forward only)
    block.eval()
    with torch.no_grad():
        e_f, _ = block(feats, pooled, adj)
    assert torch.isfinite(e_f).all()


@pytest.mark.parametrize("mesh", ["uv_sphere_482", "icosphere_162", "irregular"])
def test_tapped_layer_output_sums_its_two_gradients_in_the_batchnorm_backward(gpu, mesh):
    """A BatchNorm output that feeds the next layer AND a later residual average is handed out as two tensor objects over
    the same memory (`tap`); their two upstream gradients are added inside `geom_vertex_bn_bwd_f32` (grad_out2) instead of
    by autograd's accumulation pass.  Against the untapped layer given the pre-added gradient: outputs, running
    statistics and every gradient BIT for bit (one fp32 add either way) -- at the reference's training shape (16 x 482
    vertices, two 33-entry pole rows -> table + CSR tail in the aggregation), on a pole-free mesh (48 columns x 5 rows: the
    float4 BN kernels as well -- the scalar backward with a second gradient is held in tests/test_vertex_bn_gpu.py), and on an
    adjacency with irregular degrees (generic aggregation kernel)."""
    import copy
    from geometrics_amd import meshgen, models
    torch.manual_seed(11)
    if mesh == "irregular":
        nv, batch, hidden = 40, 3, 24
        a = (torch.rand(nv, nv) < 0.5).float()
        a = ((a + a.t()) > 0).float()
        a.fill_diagonal_(1.0)
        adj = (a / a.sum(1, keepdim=True)).to(gpu)
        assert layers.adjacency_csr(adj).ell_w == 0
    else:
        V, Fc = meshgen.uv_sphere() if mesh == "uv_sphere_482" else meshgen.icosphere(2)
        nv, batch, hidden = V.shape[0], (16 if mesh == "uv_sphere_482" else 5), (192 if mesh == "uv_sphere_482" else 48)
        adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
        csr = layers.adjacency_csr(adj)
        assert csr.ell_w == 8 and bool(csr.over) == (mesh == "uv_sphere_482")
    block = models.BatchMeshDeformationBlock(hidden + 7, nv, hidden=hidden).to(gpu).train()
    with torch.no_grad():
        block.bn4.weight.uniform_(0.5, 1.5), block.bn4.bias.uniform_(-0.3, 0.3)
    twin = copy.deepcopy(block)
    x = torch.randn(batch, nv, hidden, device=gpu)
    res = torch.randn(batch, nv, hidden, device=gpu)
    g_a, g_b = torch.randn_like(x), torch.randn_like(x)

    x1, r1 = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    y, y_again = block._layer(4, x1, adj, residual=r1, tap=True)
    assert y.data_ptr() == y_again.data_ptr() and y is not y_again and type(y.grad_fn).__name__ == "_VertexBNBackward"
    ((y * g_a).sum() + (y_again * g_b).sum()).backward()

    x2, r2 = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    z = twin.bn4(twin.gc4(x2, adj, models._identity), relu=True, residual=r2)
    z.backward(g_a + g_b)

    assert torch.equal(y, z)
    assert torch.equal(x1.grad, x2.grad) and torch.equal(r1.grad, r2.grad)
    for (name, p), (_, q) in zip(block.named_parameters(), twin.named_parameters()):
        if name.startswith(("gc4.", "bn4.")):
            assert torch.equal(p.grad, q.grad), name
    assert torch.equal(block.bn4.running_mean, twin.bn4.running_mean) and torch.equal(block.bn4.running_var, twin.bn4.running_var)
    assert int(block.state_dict()["bn4.num_batches_tracked"]) == 1
    # only ONE of the two handles used downstream
    x3 = x.clone().requires_grad_(True)
    block._layer(3, x3, adj, tap=True)[1].backward(g_a)
    x4 = x.clone().requires_grad_(True)
    twin.bn3(twin.gc3(x4, adj, models._identity), relu=True).backward(g_a)
    assert torch.equal(x3.grad, x4.grad) and torch.equal(block.gc3.bias.grad, twin.gc3.bias.grad)
    # library route (b*c > 4096 values per vertex): the same tensor twice, autograd adds
    big = torch.randn(4096 // hidden + 1, nv, hidden, device=gpu, requires_grad=True)
    o1, o2 = block._layer(5, big, adj, tap=True)
    assert o1 is o2


def test_bias_gradients_of_a_backward_pass_are_finished_in_one_batched_launch(gpu):
    """Inside an autograd pass the per-layer bias-gradient reductions are queued and finished by ONE
    geom_colsum_batch_f32 launch at the end of the pass (layers.deferred_parameter_gradients()): same bits as the immediate
    reduction, complete when backward() returns, nothing left pending; a bias with an existing .grad (accumulation) or a
    hook takes the immediate path; torch.autograd.grad sees finished values; and a captured pass replays."""
    from geometrics_amd import meshgen
    torch.manual_seed(21)
    V, Fc = meshgen.uv_sphere()
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    stack = [layers.Batch_Image_ZERON_GCNGCN(40, 48), layers.Batch_Image_ZERON_GCNGCN(48, 48), layers.BatchZERON_GCN(48, 40)]
    stack = torch.nn.ModuleList(stack).to(gpu)
    x = torch.randn(5, V.shape[0], 40, device=gpu)
    g_out = torch.randn(5, V.shape[0], 40, device=gpu)

    def run(defer, prepare=None):
        with layers.deferred_parameter_gradients(defer):
            for p in stack.parameters():
                p.grad = None
            if prepare:
                prepare()
            h = x
            for i, layer in enumerate(stack):
                h = layer(h, adj, F.relu if i < 2 else None)
            h.backward(g_out)
            assert not backward_pass.pending()
            return [layer.bias.grad.clone() for layer in stack], [layer._weight().grad.clone() for layer in stack]

    now_b, now_w = run(False)
    later_b, later_w = run(True)
    for a, b in zip(now_b + now_w, later_b + later_w):      # the end-of-pass launch adds the same partials in its own fixed
        close(b.cpu().numpy(), a.cpu().numpy(), 2e-6)       # order (one launch for bias AND weight gradients): round-off only
    again_b, again_w = run(True)
    for a, b in zip(later_b + later_w, again_b + again_w):  # and it is reproducible bit for bit
        assert torch.equal(a, b)
    close(later_b[2].cpu().numpy(), g_out.sum((0, 1)).cpu().numpy(), 1e-4)       # last layer, no activation: plain column sums

    def existing_grads():                                  # accumulation into an existing .grad reads the gradient at once
        for layer in stack:
            layer.bias.grad = torch.ones_like(layer.bias)
    acc_b, _ = run(True, existing_grads)
    for a, b in zip(acc_b, now_b):
        assert torch.equal(a, b + 1.0)
    seen = []
    hook = stack[1].bias.register_hook(lambda gr: seen.append(gr.clone()))       # a hook reads it inside the pass
    hook_b, _ = run(True)
    hook.remove()
    assert torch.equal(seen[0], now_b[1]) and torch.equal(hook_b[1], now_b[1])
    for a, b in zip(hook_b, now_b):
        close(a.cpu().numpy(), b.cpu().numpy(), 2e-6)
    # a bias shared by two layers: the engine adds the two gradients inside the pass, so neither may be postponed
    tied = layers.Batch_Image_ZERON_GCNGCN(48, 48).to(gpu)
    tied.bias = stack[1].bias
    def tied_pass(defer):
        with layers.deferred_parameter_gradients(defer):
            for p_ in list(stack.parameters()) + [tied.weight1]:
                p_.grad = None
            h = stack[0](x, adj, F.relu)
            h = tied(stack[1](h, adj, F.relu), adj, F.relu)
            stack[2](h, adj, None).backward(g_out)
            assert not backward_pass.pending()
            return stack[1].bias.grad.clone()
    assert torch.equal(tied_pass(False), tied_pass(True))      # a shared bias is never postponed: same launches either way
    del tied
    # deferral is opt-in: by default nothing is pending at any time and the values are the same
    assert backward_pass.switches.defer is False
    # torch.autograd.grad: captured gradients are finished when the call returns
    with layers.deferred_parameter_gradients():
        h = x
        for i, layer in enumerate(stack):
            h = layer(h, adj, F.relu if i < 2 else None)
        got = torch.autograd.grad(h, [layer.bias for layer in stack], g_out)
    assert not backward_pass.pending()
    for a, b in zip(got, now_b):
        close(a.cpu().numpy(), b.cpu().numpy(), 2e-6)
    # HIP-graph capture of forward + backward: the batched launch is part of the graph
    for p in stack.parameters():
        p.grad = None
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            for p in stack.parameters():
                p.grad = None
            h = static_x
            for i, layer in enumerate(stack):
                h = layer(h, adj, F.relu if i < 2 else None)
            h.backward(g_out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    for p in stack.parameters():
        p.grad = None
    with layers.deferred_parameter_gradients(), torch.cuda.graph(graph):
        h = static_x
        for i, layer in enumerate(stack):
            h = layer(h, adj, F.relu if i < 2 else None)
        h.backward(g_out)
    static_x.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    close(stack[2].bias.grad.cpu().numpy(), g_out.sum((0, 1)).cpu().numpy(), 1e-4)
    assert not torch.equal(stack[0].bias.grad, now_b[0]) and torch.isfinite(stack[0].bias.grad).all()


def test_a_layer_applied_twice_keeps_both_gradients_under_bound_gradient_targets(gpu):
    """dist.GradBucket(bind=True) hands the layers' launches the bucket view as the gradient's memory.  A parameter fed
    by TWO live autograd nodes (one layer applied twice: shared weight and bias) gets its two gradients ADDED by the engine,
    so each node must write memory of its own -- with one shared target the second node would overwrite the first's values
    before the sum is formed (round-3 advice).  Bound and unbound runs must agree, with and without deferral."""
    from geometrics_amd import dist as gdist, meshgen
    torch.manual_seed(5)
    V, Fc = meshgen.icosphere(2)
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    layer = layers.Batch_Image_ZERON_GCNGCN(192, 192).to(gpu)
    head = layers.Batch_Image_ZERON_GCNGCN(192, 192).to(gpu)
    x = torch.randn(8, V.shape[0], 192, device=gpu)
    g_out = torch.randn(8, V.shape[0], 192, device=gpu)
    params = list(layer.parameters()) + list(head.parameters())

    def run(defer):
        for p_ in params:
            p_.grad = None
        with layers.deferred_parameter_gradients(defer):
            h = layer(layer(x, adj, F.relu), adj, F.relu)          # the same layer twice
            head(h, adj, F.relu).backward(g_out)
        return [p_.grad.clone() for p_ in params]

    plain = run(False)
    bucket = gdist.GradBucket(params, extra=2, bind=True)
    try:
        for defer in (False, True):
            bound = run(defer)
            bucket.pack(torch.tensor(1.0, device=gpu), torch.tensor(2.0, device=gpu))
            for want, got, view in zip(plain, bound, bucket.views):
                close(got.cpu().numpy(), want.cpu().numpy(), 2e-6)
                assert torch.equal(view, got)                      # and pack() gathered what did not land in the view
    finally:
        layers.bind_gradient_targets(params, [None] * len(params))


def test_late_input_gradient_is_the_same_product_issued_behind_the_reduction_launch(gpu):
    """layers.late_input_gradients(): the first layer's input gradient dX = G . W^T (its consumer is a LEAF's .grad) is
    launched by the end-of-pass callback, AFTER the reduction launch that finishes the parameter gradients and after the
    `on_parameter_gradients` callback (where a data-parallel step records the event its all-reduce waits for).  Same
    product, same library kernel: bit-identical to the immediate path; the callback runs exactly once per pass, with every
    parameter gradient of the pass already launched; a leaf with a hook or an existing .grad takes the immediate path."""
    torch.manual_seed(11)
    V, Fc = meshgen.icosphere(3)
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    stack = torch.nn.ModuleList([layers.Batch_Image_ZERON_GCNGCN(963, 192), layers.Batch_Image_ZERON_GCNGCN(192, 192)]).to(gpu)
    x = torch.randn(4, V.shape[0], 963, device=gpu, requires_grad=True)
    g_out = torch.randn(4, V.shape[0], 192, device=gpu)
    calls = []

    def run(late, prepare=None):
        for p_ in stack.parameters():
            p_.grad = None
        x.grad = None
        calls.clear()
        if prepare:
            prepare()
        hook = lambda: calls.append(backward_pass.pending("reduces", "colsums"))
        with layers.deferred_parameter_gradients(), layers.late_input_gradients(hook, enabled=late):
            stack[1](stack[0](x, adj, F.relu), adj, F.relu).backward(g_out)
        assert not backward_pass.pending()
        return x.grad.clone(), [p_.grad.clone() for p_ in stack.parameters()]

    now_x, now_p = run(False)
    assert calls == [0]                                   # the callback still runs once per pass (the event must be recorded)
    late_x, late_p = run(True)
    assert calls == [0]                                   # ... with nothing left pending: the reduction launch is out
    assert torch.equal(late_x, now_x)
    for a, b in zip(late_p, now_p):
        assert torch.equal(a, b)
    seen = []
    h = x.register_hook(lambda gr: seen.append(gr.clone()))
    hook_x, _ = run(True)                                 # somebody reads the gradient inside the pass: immediate product
    h.remove()
    assert torch.equal(seen[0], now_x) and torch.equal(hook_x, now_x)
    acc_x, _ = run(True, lambda: setattr(x, "grad", torch.ones_like(x)))     # accumulation reads it at once too
    assert torch.equal(acc_x, now_x + 1.0)
    # (round-4 advice) a leaf with SEVERAL consumers: the postponing node gives the engine no gradient for the leaf at all;
    # the end-of-pass callback adds its product to whatever the other consumers contributed through the engine
    twin = layers.Batch_Image_ZERON_GCNGCN(963, 192).to(gpu)

    def both(late):
        x.grad = None
        for p_ in list(stack.parameters()) + list(twin.parameters()):
            p_.grad = None
        with layers.deferred_parameter_gradients(), layers.late_input_gradients(enabled=late):
            (stack[0](x, adj, F.relu) + twin(x, adj, F.relu)).backward(g_out)
        return x.grad.clone()
    close(both(True).cpu().numpy(), both(False).cpu().numpy(), 1e-6)     # (two postponed products are added in another order)

    def with_torch_op(late):                              # ... and a consumer this module cannot see: a plain torch op on the leaf
        x.grad = None
        with layers.deferred_parameter_gradients(), layers.late_input_gradients(enabled=late):
            ((stack[0](x, adj, F.relu) * g_out).sum() + (x * 2.0).sum()).backward()
        return x.grad.clone()
    close(with_torch_op(True).cpu().numpy(), with_torch_op(False).cpu().numpy(), 1e-6)
    assert float((with_torch_op(True) - 2.0).abs().max()) > 0.0 and not backward_pass.pending()


def test_weight_gradients_of_equal_layers_come_from_one_batched_product(gpu):
    """Inside layers.weight_gradient_batching() the weight gradients of a stack are postponed to the end of the backward
    pass and runs of equal layers are issued as ONE strided-batched product over stacked activation / gradient buffers:
    same values as the per-layer products up to the library kernel's summation order, every other gradient and the
    outputs bit-identical; the operands of the run really sit at a regular pitch; an existing .grad (accumulation) takes
    the immediate product; the deformation block uses it by itself."""
    from geometrics_amd import meshgen, models
    torch.manual_seed(31)
    V, Fc = meshgen.uv_sphere()
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    widths = ((40, 48), (48, 48), (48, 48), (48, 48), (48, 40))
    stack = torch.nn.ModuleList([layers.Batch_Image_ZERON_GCNGCN(i, o) for i, o in widths]).to(gpu)
    x = torch.randn(6, V.shape[0], 40, device=gpu, requires_grad=True)
    g_out = torch.randn(6, V.shape[0], 40, device=gpu)

    def run(batched, prepare=None):
        for p in stack.parameters():
            p.grad = None
        x.grad = None
        if prepare:
            prepare()
        ctxm = layers.weight_gradient_batching() if batched else contextlib.nullcontext()
        with ctxm:
            h = x
            for i, layer in enumerate(stack):
                h = layer(h, adj, F.relu if i < 4 else None)
        h.backward(g_out)
        assert not backward_pass.pending()
        return (h.detach().clone(), x.grad.clone(), [l.weight1.grad.clone() for l in stack], [l.bias.grad.clone() for l in stack])

    import contextlib
    seen = []
    real_bmm = torch.bmm
    def spy(a, b, out=None):
        seen.append((tuple(a.shape), tuple(a.stride()), tuple(b.stride())))
        return real_bmm(a, b, out=out)
    plain = run(False)
    torch.bmm = spy
    try:
        batched = run(True)
    finally:
        torch.bmm = real_bmm
    assert seen == [((3, 48, 6 * V.shape[0]), seen[0][1], seen[0][2])] and seen[0][1][0] > 0 and seen[0][2][0] > 0   # ONE product for the three 48 x 48 layers
    assert torch.equal(plain[0], batched[0])
    close(batched[1].cpu().numpy(), plain[1].cpu().numpy(), 2e-5)   # input gradient: matrix-core kernel vs library product
    for a, b in zip(plain[3], batched[3]):      # bias gradients: downstream of the input gradients (matrix-core kernel vs library)
        close(b.cpu().numpy(), a.cpu().numpy(), 2e-5)
    for a, b in zip(plain[2], batched[2]):
        assert a.shape == b.shape
        close(b.cpu().numpy(), a.cpu().numpy(), 2e-5)
    def existing():
        stack[2].weight1.grad = torch.ones_like(stack[2].weight1)
    acc = run(True, existing)
    close(acc[2][2].cpu().numpy(), (plain[2][2] + 1.0).cpu().numpy(), 2e-5)
    close(acc[2][1].cpu().numpy(), plain[2][1].cpu().numpy(), 2e-5)
    # the deformation block batches its twelve hidden layers without being asked
    block = models.BatchMeshDeformationBlock(60, V.shape[0], hidden=48).to(gpu).train()
    feats, pooled = torch.randn(4, V.shape[0], 3, device=gpu, requires_grad=True), torch.randn(4, V.shape[0], 57, device=gpu, requires_grad=True)
    seen.clear()
    torch.bmm = spy
    try:
        f, coords = block(feats, pooled, adj)
        (f.sum() + coords.sum()).backward()
    finally:
        torch.bmm = real_bmm
    assert len(seen) == 1 and seen[0][0][0] == 12
    assert all(torch.isfinite(p.grad).all() for n, p in block.named_parameters() if not n.startswith("bn14"))


def test_block_input_tap_equals_cat_and_slice(gpu):
    """models._InputTap (cat + the leading columns as a contiguous second output, narrow gradient added in place) against
    torch.cat + a slice: same values, same gradients, for 3 + 1152 columns / 192 hidden and for a feature part WIDER than
    the hidden width."""
    from geometrics_amd import models
    torch.manual_seed(5)
    for nf, npool, width in ((3, 1152, 192), (40, 30, 24), (3, 21, 24)):
        f = torch.randn(4, 37, nf, device=gpu)
        p = torch.randn(4, 37, npool, device=gpu)
        ga, gb = torch.randn(4, 37, nf + npool, device=gpu), torch.randn(4, 37, width, device=gpu)
        f1, p1 = f.clone().requires_grad_(True), p.clone().requires_grad_(True)
        full, lead = models._InputTap.apply(f1, p1, width)
        assert lead.is_contiguous()
        ((full * ga).sum() + (lead * gb).sum()).backward()
        f2, p2 = f.clone().requires_grad_(True), p.clone().requires_grad_(True)
        full2 = torch.cat((f2, p2), dim=-1)
        ((full2 * ga).sum() + (full2[..., :width] * gb).sum()).backward()
        assert torch.equal(full, full2) and torch.equal(lead, full2[..., :width])
        assert torch.equal(f1.grad, f2.grad) and torch.equal(p1.grad, p2.grad)
        f3 = f.clone().requires_grad_(True)                   # only the narrow output used, only one input differentiable
        models._InputTap.apply(f3, p, width)[1].backward(gb)
        exp = torch.zeros_like(f)
        exp[..., :min(nf, width)] = gb[..., :min(nf, width)]
        assert torch.equal(f3.grad, exp)


def test_vertex_batchnorm_matches_torch(gpu):
    from geometrics_amd import models
    torch.manual_seed(2)
    bn, ref = models.VertexBatchNorm(50).to(gpu), torch.nn.BatchNorm1d(50).to(gpu)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 2), bn.bias.uniform_(-1, 1)
        ref.weight.copy_(bn.weight), ref.bias.copy_(bn.bias)
    x = torch.randn(4, 50, 36, device=gpu, requires_grad=True)
    wide = torch.randn(4, 50, 60, device=gpu, requires_grad=True)
    xr, wr = x.detach().clone().requires_grad_(True), wide.detach().clone().requires_grad_(True)
    out = bn(x, relu=True, residual=wide[:, :, :36])         # residual = column slice of a wider tensor
    exp = (wr[:, :, :36] + torch.relu(ref(xr))) / 2
    g = torch.randn_like(out)
    out.backward(g)
    exp.backward(g)
    close(out.detach().cpu().numpy(), exp.detach().cpu().numpy(), 1e-5)
    close(x.grad.cpu().numpy(), xr.grad.cpu().numpy(), 1e-4)
    close(wide.grad.cpu().numpy(), wr.grad.cpu().numpy(), 1e-5)
    close(bn.weight.grad.cpu().numpy(), ref.weight.grad.cpu().numpy(), 1e-4)
    close(bn.bias.grad.cpu().numpy(), ref.bias.grad.cpu().numpy(), 1e-4)
    close(bn.running_var.cpu().numpy(), ref.running_var.cpu().numpy(), 1e-5)
    bn.eval(), ref.eval()
    with torch.no_grad():
        close(bn(x).cpu().numpy(), ref(x).cpu().numpy(), 1e-5)
    big = torch.randn(30, 50, 192, device=gpu)                # b*c > 4096: library-op route, same result
    bn.train(), ref.train()
    close(bn(big, relu=True).detach().cpu().numpy(), torch.relu(ref(big)).detach().cpu().numpy(), 1e-5)


def test_batched_pooling_matches_reference_fixture(gpu):
    """camera projection + bilinear pooling of four feature maps, forward and the
    gradients w.r.t. the maps and the vertex positions, against the reference's own batched_pooling."""
    g = golden("pooling_v162")
    cam_mat, cam_pos = utils.batch_camera_info(dev(g["img_info"], gpu))
    close(cam_mat.cpu().numpy(), g["cam_mat"], 1e-6)
    close(cam_pos.cpu().numpy(), g["cam_pos"], 1e-6)
    blocks = [dev(g["block%d" % i], gpu, grad=True) for i in range(4)]
    verts = dev(g["verts"], gpu, grad=True)
    feats = utils.batched_pooling(blocks, verts, dev(g["img_info"], gpu))
    assert feats.shape == (2, 162, 36)
    # the pixel coordinate is scaled by the map resolution (up to 56), which amplifies the fp32 round-off of
    # the projection (the reference's own matmul order is BLAS-dependent); the maps here are white noise
    close(feats.detach().cpu().numpy(), g["features"], 3e-5)
    # the camera formed once and handed over (a driver that pools several times per step with the same cameras): same bits
    assert torch.equal(utils.batched_pooling(blocks, verts, (cam_mat, cam_pos)), feats)
    feats.backward(dev(g["grad_out"], gpu))
    for i, blk in enumerate(blocks):
        close(blk.grad.cpu().numpy(), g["grad_block%d" % i], 3e-5)
    close(verts.grad.cpu().numpy(), g["grad_verts"], 2e-4)
    # clamped vertices exist in the fixture (zero position gradient through the clamp) and are reproduced
    assert (np.abs(g["grad_verts"]).sum(-1) == 0).any()


def test_camera_kernel_against_the_torch_expressions(gpu):
    """utils.batch_camera_info on device parameters is ONE launch (geom_camera_info_f32) evaluating the reference's
    expressions (utils.py:286-313) in the same order; against the torch-op form of the same lines (what a parameter tensor
    that requires a gradient still takes), negative and > 360 degree angles included (the `%` is torch.remainder)."""
    torch.manual_seed(12)
    param = torch.stack((torch.rand(64) * 1200 - 400, torch.rand(64) * 160 - 80, torch.rand(64) * 2 + 0.5), dim=1).to(gpu)
    cam_mat, cam_pos = utils.batch_camera_info(param)
    ref_mat, ref_pos = utils.batch_camera_info(param.clone().requires_grad_(True))       # the torch expressions
    close(cam_mat.cpu().numpy(), ref_mat.detach().cpu().numpy(), 2e-6)
    close(cam_pos.cpu().numpy(), ref_pos.detach().cpu().numpy(), 2e-6)
    eye = torch.matmul(cam_mat, cam_mat.transpose(1, 2)).cpu()
    assert float((eye - torch.eye(3)).abs().max()) < 1e-5                                 # orthonormal rows


def test_pooling_with_more_channel_chunks_than_grid_slices(gpu):
    """The pooling launches give every workgroup one 64-channel chunk up to 32 chunks; beyond that a workgroup walks several
    (and sums their shares of the vertex gradient).  Two maps of 1280 channels = 40 chunks against the same maps pooled in
    halves of 640 (10 + 10 chunks per call): features per channel bit for bit, map gradients and the vertex gradient (= the sum
    of the halves') within fp32 round-off -- and the vertex gradient element by element against the float64 closed form."""
    torch.manual_seed(12)
    V, _ = meshgen.icosphere(2)
    b, nv = 2, V.shape[0]
    verts = dev(meshgen.jittered_batch(V, b), gpu, grad=True)
    img_info = torch.tensor([[35.0, 20.0, 1.2], [60.0, 30.0, 1.0]], device=gpu)
    big = [torch.randn(b, 1280, d, d, device=gpu, requires_grad=True) for d in (14, 7)]
    grad_out = torch.randn(b, nv, 2560, device=gpu)
    feats = utils.batched_pooling(big, verts, img_info.clone())
    assert feats.shape == (b, nv, 2560)
    feats.backward(grad_out)
    gv_big, gmaps_big = verts.grad.clone(), [m.grad.clone() for m in big]
    verts.grad = None
    gv_sum = torch.zeros_like(gv_big)
    for half in range(2):
        sl = slice(640 * half, 640 * (half + 1))
        parts = [m.detach()[:, sl].contiguous().requires_grad_(True) for m in big]
        f = utils.batched_pooling(parts, verts, img_info.clone())
        cols = torch.cat([torch.arange(1280 * i + 640 * half, 1280 * i + 640 * (half + 1)) for i in range(2)]).to(gpu)
        assert torch.equal(f, feats.detach()[..., cols])
        f.backward(grad_out[..., cols].contiguous())
        for i in range(2):      # (a texel's contributions are listed in arrival order: same terms, fp32 summation order may differ)
            close(parts[i].grad.cpu().numpy(), gmaps_big[i][:, sl].cpu().numpy(), 2e-6)
        gv_sum += verts.grad
        verts.grad = None
    close(gv_big.cpu().numpy(), gv_sum.cpu().numpy(), 2e-5)
    cam_mat, cam_pos = utils.batch_camera_info(img_info.clone())
    pool_vertex_gradient_close(gv_big, big, verts, cam_mat, cam_pos, grad_out, "pooling verts.grad 40 chunks (device-drawn maps)")


def test_surface_loss_with_per_mesh_weights_equals_the_weighted_stages(gpu):
    """batch_point_to_surface(weight=[B] tensor): three 'stages' of 5 meshes stacked into one call against one ground truth,
    factors 3 x (.2, .2, 2) per stage (the mean runs over the stacked batch) -- loss and position gradients against the three
    separate calls `w_s * batch_point_to_surface(stage s)` on the SAME draws (GEOMetrics.py:134-138).  The stacked call forms
    the same per-point terms (the factor enters the loss's summation and, in the backward, scales the finished per-vertex
    sum): agreement to fp32 round-off of the differently grouped sums."""
    torch.manual_seed(41)
    V, Fc = meshgen.icosphere(2)
    nb, num = 5, 700
    faces = dev(Fc, gpu)
    info = utils.adj_init(faces)
    stages = [dev(meshgen.jittered_batch(V, nb, first=10 * k), gpu, grad=True) for k in range(3)]
    gt = dev(meshgen.gt_cloud(nb, 900, first=3), gpu)
    ops.manual_seed(77, gpu)
    draws = [ops.draw_samples(p.detach(), faces, num)[:3] for p in stages]
    ws = (.2, .2, 2.0)
    ref_loss = 0.0
    for p, d, w in zip(stages, draws, ws):
        term = w * utils.batch_point_to_surface(p, info, gt, num=num, draws=d)
        term.backward()
        ref_loss = ref_loss + term.detach().double()
    ref_grads = [p.grad.clone() for p in stages]
    for p in stages:
        p.grad = None
    stacked = torch.cat(stages).detach().requires_grad_(True)
    weight = torch.tensor([3 * w for w in ws for _ in range(nb)], dtype=torch.float32, device=gpu)
    all_draws = tuple(torch.cat([d[k] for d in draws]) for k in range(3))
    loss = utils.batch_point_to_surface(stacked, info, torch.cat((gt, gt, gt)), num=num, draws=all_draws, weight=weight)
    loss.backward()
    assert abs(float(loss.detach().double() - ref_loss)) <= 2e-6 * abs(float(ref_loss))
    for k in range(3):
        close(stacked.grad[k * nb:(k + 1) * nb].cpu().numpy(), ref_grads[k].cpu().numpy(), 2e-6)
    # an upstream factor and a constant weight vector: the scalar route's result
    stacked.grad = None
    ones = torch.full((3 * nb,), 1.5, device=gpu)
    (2.0 * utils.batch_point_to_surface(stacked, info, torch.cat((gt, gt, gt)), num=num, draws=all_draws, weight=ones)).backward()
    g_vec = stacked.grad.clone()
    stacked.grad = None
    (2.0 * utils.batch_point_to_surface(stacked, info, torch.cat((gt, gt, gt)), num=num, draws=all_draws, weight=1.5)).backward()
    close(g_vec.cpu().numpy(), stacked.grad.cpu().numpy(), 2e-6)
    with pytest.raises(RuntimeError):
        utils.batch_point_to_surface(stacked, info, torch.cat((gt, gt, gt)), num=num, weight=weight[:4])


def _pooling_against_float64(gpu, verts, img_info, chans, dims, headrooms=(0,)):
    """forward and map gradient of batched_pooling against float64 built from the pooling operator itself: pooling identity
    maps (channel t = the one-hot map of texel t) returns P [b, nv, texels] with the weights as the kernel forms them, so
    feats = P maps and d maps = P^T g in float64, per element, bound 8 eps * sum |P||g| (|maps|).  (P itself and the vertex
    gradient against the float64 restatement of the reference: test_pooling_vertex_gradient_gpu.py.)"""
    b = verts.shape[0]
    maps = [torch.randn(b, c, d, d, device=gpu, requires_grad=True) for c, d in zip(chans, dims)]
    eps = np.finfo(np.float32).eps
    Ps = []
    for d in dims:
        eye = torch.eye(d * d, device=gpu).view(1, d * d, d, d).expand(b, -1, -1, -1).contiguous()
        Ps.append(utils.batched_pooling([eye], verts, img_info.clone()).double())                  # [b, nv, d*d]
    for headroom in headrooms:
        feats = utils.batched_pooling(maps, verts, img_info.clone(), headroom=headroom)
        g = torch.randn_like(feats)
        grads = torch.autograd.grad(feats, maps, g)
        col = 0
        for c, d, P, m, got in zip(chans, dims, Ps, maps, grads):
            md = m.detach().double().view(b, c, d * d)
            ref_f = torch.einsum("bvt,bct->bvc", P, md)
            bound_f = 8 * eps * torch.einsum("bvt,bct->bvc", P.abs(), md.abs()) + 1e-30
            err_f = (feats.detach()[..., col:col + c].double() - ref_f).abs()
            assert bool((err_f <= bound_f).all()), "features of map %d x %d: err/bound up to %.3g" % (d, d, float((err_f / bound_f).max()))
            gl = g[..., col:col + c].double()
            ref = torch.einsum("bvt,bvc->bct", P, gl).view(b, c, d, d)
            bound = 8 * eps * torch.einsum("bvt,bvc->bct", P.abs(), gl.abs()).view(b, c, d, d) + 1e-30
            err = (got.double() - ref).abs()
            assert bool((err <= bound).all()), "map %d x %d: err/bound up to %.3g" % (d, d, float((err / bound).max()))
            col += c
    return Ps


def test_pooling_at_ragged_shapes_per_element(gpu):
    """Channel counts that are no multiple of 64 (or of the lane vector: 70 -> 1, 130 -> 2, 260 -> 4 channels per lane, a
    partial last slice each), map sizes 1 x 1 (every weight zero: integral coordinate), 2 x 2, odd sizes whose runs end
    ragged, one map larger than a run's tile allows 64 texels for (260 channels x 40 x 40), a vertex count that is no
    multiple of the 64-vertex tile, vertices that project outside the image (clamped)."""
    torch.manual_seed(32)
    V, _ = meshgen.icosphere(1)                                                     # 42 vertices
    V = np.concatenate([V, 0.5 * V, 2.5 * V], 0)[:101]                              # (2.5 x: outside the image for some cameras)
    verts = dev(meshgen.jittered_batch(V, 2), gpu)
    img_info = torch.tensor([[35.0, 20.0, 1.2], [250.0, -30.0, 0.8]], device=gpu)
    _pooling_against_float64(gpu, verts, img_info, chans=(70, 130, 260, 5), dims=(5, 9, 40, 1), headrooms=(0, 7))
    _pooling_against_float64(gpu, verts, img_info, chans=(3, 64), dims=(2, 13))


def test_pooling_map_gradient_per_element_at_the_training_shape(gpu):
    """d loss / d maps at the reference's training shape (482 vertices, the four VGG maps 64 x 56^2 ... 512 x 7^2), every
    element against float64.  The pooling is LINEAR in the maps: feats[b, v, c] = sum_t P_b[v, t] map[b, c, t], and pooling
    identity maps (channel t = the one-hot map of texel t) returns P itself with the weights as the kernel forms them -- so
    the gradient is P^T g in float64, with the per-element bound 8 eps * sum |P||g| (a texel's list holds 1 ... ~60 terms).
    Exercises all four run lengths of the gather (64 / 16 / 4 / 1 texels per workgroup), ragged last runs and -- on a buffer
    with headroom -- the pitched read of the gradient."""
    torch.manual_seed(31)
    b, chans, dims = 3, (64, 128, 256, 512), (56, 28, 14, 7)
    V, _ = meshgen.icosphere(2)
    V = np.concatenate([V, 0.6 * V, 0.3 * V], 0)[:482]                 # 482 vertices at three radii
    verts = dev(meshgen.jittered_batch(V, b), gpu)
    img_info = torch.tensor([[35.0, 20.0, 1.2], [200.0, -10.0, 1.0], [310.0, 45.0, 1.4]], device=gpu)
    maps = [torch.randn(b, c, d, d, device=gpu, requires_grad=True) for c, d in zip(chans, dims)]
    for headroom in (0, 195):
        feats = utils.batched_pooling(maps, verts, img_info.clone(), headroom=headroom)
        g = torch.randn_like(feats)
        grads = torch.autograd.grad(feats, maps, g)
        col = 0
        for c, d, got in zip(chans, dims, grads):
            eye = torch.eye(d * d, device=gpu).view(1, d * d, d, d).expand(b, -1, -1, -1).contiguous()
            P = utils.batched_pooling([eye], verts, img_info.clone()).double()                      # [b, nv, d*d]
            gl = g[..., col:col + c].double()
            ref = torch.einsum("bvt,bvc->bct", P, gl).view(b, c, d, d)
            bound = 8 * np.finfo(np.float32).eps * torch.einsum("bvt,bvc->bct", P.abs(), gl.abs()).view(b, c, d, d) + 1e-30
            err = (got.double() - ref).abs()
            assert bool((err <= bound).all()), "map %d x %d: err/bound up to %.3g" % (d, d, float((err / bound).max()))
            assert bool((ref == 0).any()) or d < 28          # texels nothing projects into are written as zeros
            col += c


def test_in_kernel_sampler_stream(gpu):
    """The Philox stream of the sampler: reproducible after manual_seed, fresh numbers on every call (also
    when the call is replayed from a HIP graph), uniform u/v, area-weighted faces."""
    V, Fc = meshgen.icosphere(3)
    verts, faces = dev(meshgen.jittered_batch(V, 2), gpu), dev(Fc, gpu)
    ops.manual_seed(123)
    c1, u1, v1 = ops.draw_samples(verts, faces, 5000)
    c2, u2, v2 = ops.draw_samples(verts, faces, 5000)
    assert not torch.equal(c1, c2) and not torch.equal(u1, u2)                  # the stream advances
    ops.manual_seed(123)
    c3, u3, v3 = ops.draw_samples(verts, faces, 5000)
    assert torch.equal(c1, c3) and torch.equal(u1, u3) and torch.equal(v1, v3)  # and is reproducible
    assert not torch.equal(c1[0], c1[1])                                        # meshes draw independently
    graph = torch.cuda.CUDAGraph()
    ops.draw_samples(verts, faces, 5000)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        cg, ug, vg = ops.draw_samples(verts, faces, 5000)
    graph.replay()
    first = cg.clone()
    graph.replay()
    assert not torch.equal(first, cg)                                           # replays are not frozen
    big_c, big_u, big_v = ops.draw_samples(verts, faces, 200000)
    areas = ops.face_areas(verts, faces)[0].double().cpu()
    freq = torch.bincount(big_c[0], minlength=Fc.shape[0]).double().cpu() / 200000
    assert float((freq - areas / areas.sum()).abs().max()) < 1e-3
    assert abs(float((big_u * big_u).mean()) - 0.5) < 5e-3 and abs(float(big_v.mean()) - 0.5) < 5e-3
    assert float(big_u.min()) >= 0 and float(big_u.max()) < 1 and float(big_v.max()) < 1


def test_vertex_head_matches_slice_formulation(gpu):
    base = torch.randn(3, 50, 3, device=gpu, requires_grad=True)
    feat = torch.randn(3, 50, 24, device=gpu, requires_grad=True)
    b2, f2 = base.detach().clone().requires_grad_(True), feat.detach().clone().requires_grad_(True)
    out = ops.VertexHead.apply(base, feat, 0.01)
    ref = b2 + 0.01 * f2[..., :3]
    g = torch.randn_like(out)
    out.backward(g)
    ref.backward(g)
    assert torch.allclose(out, ref, rtol=1e-6, atol=1e-7)
    assert torch.allclose(base.grad, b2.grad) and torch.allclose(feat.grad, f2.grad, rtol=1e-6, atol=1e-9)


def test_fused_draw_points_and_fused_backward_match_the_separate_kernels(gpu):
    """utils.batch_point_to_surface with its own draws uses (a) the draw kernel's points output and (b) the one-launch
    backward; both must give the bits of the separate gather / two-scatter formulation on the same draws."""
    V, Fc = meshgen.icosphere(3)
    verts = dev(meshgen.jittered_batch(V, 3), gpu).requires_grad_(True)
    faces, gt = dev(Fc, gpu), dev(meshgen.gt_cloud(3, 700), gpu)
    ops.manual_seed(5)
    choices, u, v, points = ops.draw_samples(verts, faces, 900, with_points=True)
    assert torch.equal(points, ops.SampleFaces.apply(verts, faces, choices, u, v).detach())
    loss_a, sq_gt_a, sq_pred_a = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, 3000.0, points)
    loss_a.backward()
    grad_a, verts.grad = verts.grad.clone(), None
    loss_b, sq_gt_b, sq_pred_b = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, 3000.0)
    loss_b.backward()
    assert torch.equal(loss_a, loss_b) and torch.equal(sq_pred_a, sq_pred_b) and torch.equal(sq_gt_a, sq_gt_b)
    # atomics: the two backward formulations add the same terms in a different order
    assert torch.allclose(grad_a, verts.grad, rtol=1e-5, atol=1e-6 * float(grad_a.abs().max()))
    # the arrival counter of the sampler stream is back to zero and the position advanced by exactly one per call
    state = ops._rng_state(gpu).cpu()
    assert int(state[2]) == 0 and int(state[1]) == 1


def test_relu_sign_mask_backward_equals_the_output_based_one(gpu):
    """ELL aggregation, ReLU, split 3: the backward that takes relu' from the 1-bit-per-element mask written by the
    forward must give the bits of the backward that re-reads the forward output (and the layer must use it)."""
    from geometrics_amd import _lib as L
    V, Fc = meshgen.icosphere(3)
    adj = utils.adj_init(dev(Fc, gpu))["adj"]
    csr = layers.adjacency_csr(adj)
    B, C, k, nv = 3, 48, 16, V.shape[0]
    torch.manual_seed(1)
    sup, bias, g = torch.randn(B, nv, C, device=gpu), torch.randn(C, device=gpu), torch.randn(B, nv, C, device=gpu)
    out = torch.empty_like(sup)
    words = L.lib().geom_zn_gcn_relu_mask_words(B, nv, C, k)
    assert words == B * nv * (k // 4) and L.lib().geom_zn_gcn_relu_mask_words(B, nv, 40, 4) == 0
    mask = torch.zeros(words, dtype=torch.int16, device=gpu)
    L.call("geom_zn_gcn_aggregate_ell_fwd_f32", B, nv, C, k, csr.ell_w, csr.ell_col.data_ptr(), csr.ell_val.data_ptr(),
           None, None, None, sup.data_ptr(), bias.data_ptr(), 1, out.data_ptr(), mask.data_ptr())
    bits = (mask.view(B, nv, k // 4, 1).int() >> torch.arange(12, device=gpu).int()) & 1       # [B,nv,k/4,12]
    expect = (out > 0).view(B, nv, 3, k // 4, 4).permute(0, 1, 3, 2, 4).reshape(B, nv, k // 4, 12).int()
    assert torch.equal(bits, expect)
    scr = torch.empty(L.lib().geom_zn_gcn_bwd_scratch_floats(B, nv, C), device=gpu)
    res = []
    for use_mask in (False, True):
        gs, gb = torch.empty_like(sup), torch.empty(C, device=gpu)
        L.call("geom_zn_gcn_aggregate_ell_bwd_f32", B, nv, C, k, csr.ell_w, csr.ell_col_t.data_ptr(),
               csr.ell_val_t.data_ptr(), None, None, None, g.data_ptr(), None if use_mask else out.data_ptr(),
               mask.data_ptr() if use_mask else None, 1, gs.data_ptr(), gb.data_ptr(), scr.data_ptr())
        res.append((gs, gb))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    # the mask is a ReLU / split-3 facility: anything else is refused
    assert L.lib().geom_zn_gcn_aggregate_ell_fwd_f32(B, nv, C, k, csr.ell_w, csr.ell_col.data_ptr(), csr.ell_val.data_ptr(),
                                                     None, None, None, sup.data_ptr(), bias.data_ptr(), 2, out.data_ptr(), mask.data_ptr(),
                                                     L.stream_ptr()) == -1
    # autograd path: a ReLU layer saves the mask, not the output
    layer = layers.Batch_Image_ZERON_GCNGCN(20, C).to(gpu)
    x = torch.randn(B, nv, 20, device=gpu, requires_grad=True)
    y = layer(x, adj, torch.relu)
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].dtype == torch.int16
    y.backward(g)
    x2 = x.detach().clone().requires_grad_(True)
    ref = torch.relu(torch.cat((adj @ (x2 @ layer.weight1[0])[..., :k], (x2 @ layer.weight1[0])[..., k:]), -1) + layer.bias)
    ref.backward(g)
    assert torch.allclose(x.grad, x2.grad, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("crowded", [0.0, 0.05, 0.9])
def test_gather_backward_matches_the_atomic_scatter_and_is_reproducible(gpu, two_sided, crowded):
    """The surface-loss backward (bin by face + per-vertex gather) against the scatter kernels it replaced, called
    through the C ABI on a zeroed buffer.  crowded = share of the samples moved onto 3 faces: 0.05 gives segments of
    a few dozen points (insertion-sorted by one thread), 0.9 segments of ~180 (wave-wide rank sort).  Two runs of the
    gather give identical bits (fixed summation order)."""
    from geometrics_amd import _lib as L
    V, Fc = meshgen.icosphere(2)
    B, num, n_gt = 2, 600, 500
    verts = dev(meshgen.jittered_batch(V, B), gpu).requires_grad_(True)
    faces, gt = dev(Fc, gpu), dev(meshgen.gt_cloud(B, n_gt), gpu)
    ops.manual_seed(11)
    choices, u, v = ops.draw_samples(verts, faces, num)
    if crowded:
        choices = torch.where(torch.rand(B, num, device=gpu) < crowded, choices % 3, choices)
    grads = []
    for _ in range(2):
        verts.grad = None
        loss, _, _ = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, two_sided, 3000.0)
        loss.backward()
        grads.append(verts.grad.clone())
    assert torch.equal(grads[0], grads[1])
    # the scatter formulation on the same saved quantities
    outs = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, two_sided, 3000.0)
    saved = outs[0].grad_fn.saved_tensors
    points, idx_g = saved[4], saved[6]
    ref = torch.zeros(B, V.shape[0], 3, device=gpu)
    one = torch.ones((), device=gpu)
    args = (B, V.shape[0], Fc.shape[0], faces.data_ptr(), num, choices.data_ptr(), u.data_ptr(), v.data_ptr(),
            points.data_ptr(), n_gt, gt.data_ptr())
    L.call("geom_sample_chamfer_bwd_f32", *args, idx_g.data_ptr(), 0, one.data_ptr(), 3000.0 / (B * num), ref.data_ptr())
    if two_sided:
        L.call("geom_sample_chamfer_bwd_f32", *args, saved[7].data_ptr(), 1, one.data_ptr(), 3000.0 / (B * n_gt),
               ref.data_ptr())
    else:
        index, closest, weights = saved[7:10]
        L.call("geom_p2tri_loss_bwd_f32", B, n_gt, gt.data_ptr(), V.shape[0], Fc.shape[0], faces.data_ptr(), index.data_ptr(),
               closest.data_ptr(), weights.data_ptr(), one.data_ptr(), 3000.0 / (B * n_gt), ref.data_ptr())
    assert torch.allclose(grads[0], ref, rtol=2e-5, atol=2e-6 * float(ref.abs().max()))
    # vertex -> incident faces table: every (face, corner) exactly once, under its vertex
    vf_ptr, vf_item = ops.vertex_faces(faces, V.shape[0])
    owner = torch.repeat_interleave(torch.arange(V.shape[0], device=gpu), (vf_ptr[1:] - vf_ptr[:-1]).long())
    assert torch.equal(faces[(vf_item >> 2).long(), (vf_item & 3).long()], owner)
    assert sorted((vf_item.long() >> 2) * 3 + (vf_item.long() & 3)) == list(range(3 * Fc.shape[0]))


def test_gather_backward_at_the_reference_training_shape(gpu):
    """482 vertices / 960 faces with 3000 + 3000 points per mesh (GEOMetrics.py:25,44): ~6 points per face on average,
    dozens on the large faces, 32 incident faces at the poles -- the distribution that made the first (16 slots per
    face) binning fall back to scanning every point.  Against the atomic scatter, and bit-reproducible."""
    from geometrics_amd import _lib as L
    V, Fc = meshgen.uv_sphere()
    B, num = 4, 3000
    verts = dev(meshgen.jittered_batch(V, B, first=70), gpu).requires_grad_(True)
    faces, gt = dev(Fc, gpu), dev(meshgen.gt_cloud(B, num, first=70), gpu)
    ops.manual_seed(3)
    choices, u, v = ops.draw_samples(verts, faces, num)
    assert int(torch.bincount(choices[0], minlength=Fc.shape[0]).max()) >= 10
    grads = []
    for _ in range(2):
        verts.grad = None
        loss, _, _ = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, 3000.0)
        loss.backward()
        grads.append(verts.grad.clone())
    assert torch.equal(grads[0], grads[1])
    outs = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, 3000.0)
    saved = outs[0].grad_fn.saved_tensors
    ref = torch.zeros(B, V.shape[0], 3, device=gpu)
    one = torch.ones((), device=gpu)
    L.call("geom_surface_loss_bwd_f32", B, V.shape[0], Fc.shape[0], faces.data_ptr(), num, choices.data_ptr(), u.data_ptr(),
           v.data_ptr(), saved[4].data_ptr(), num, gt.data_ptr(), saved[6].data_ptr(), saved[7].data_ptr(),
           saved[8].data_ptr(), saved[9].data_ptr(), one.data_ptr(), 3000.0 / (B * num), 3000.0 / (B * num), ref.data_ptr())
    assert torch.allclose(grads[0], ref, rtol=2e-5, atol=2e-6 * float(ref.abs().max()))


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("fma", [False, True])
def test_fused_surface_scan_equals_the_separate_scans_and_its_records_those_of_the_finalize_pass(gpu, two_sided, fma):
    """geom_surface_scan_f32 at the BASELINE shard (8 meshes: one heterogeneous launch for the tri tiles and the NN
    tiles) against geom_chamfer_nn_f32 + geom_tri_surface_fwd_f32, bit for bit; and the gradient records its epilogues
    write against the ones the finalize pass forms from the saved tensors -- same `order` scratch, same gradient."""
    import ctypes
    from geometrics_amd import _lib as L
    from geometrics_amd.chamfer_distance import chamfer_nn
    from geometrics_amd.tri_distance import face_order, tri_distance_indexed
    lib = L.lib()
    V, Fc = meshgen.icosphere(4)
    B, num, n_gt = 8, 3000, 3000
    verts, faces, gt = dev(meshgen.jittered_batch(V, B), gpu), dev(Fc, gpu), dev(meshgen.gt_cloud(B, n_gt), gpu)
    ops.manual_seed(21)
    choices, u, v, points = ops.draw_samples(verts, faces, num, with_points=True)
    nv, nf = V.shape[0], Fc.shape[0]
    flags = L.FLAG_NN_FMA if fma else 0
    f32, i32 = dict(dtype=torch.float32, device=gpu), dict(dtype=torch.int32, device=gpu)
    order_tri = face_order(verts, faces)
    ws_bytes = lib.geom_tri_distance_workspace_bytes(B, n_gt, nf)
    coef_s, coef_o = 3000.0 / (B * num), 3000.0 / (B * n_gt)

    def run(with_records):
        o = dict(sq_gt=torch.empty(B, n_gt, **f32), idx_p=torch.empty(B, n_gt, **i32), sq_pred=torch.empty(B, num, **f32),
                 idx_g=torch.empty(B, num, **i32), tri_d=torch.empty(B, n_gt, **f32), option=torch.empty(B, n_gt, **i32),
                 index=torch.empty(B, n_gt, **i32), sq=torch.empty(B, n_gt, **f32), closest=torch.empty(B, n_gt, 3, **f32),
                 weights=torch.empty(B, n_gt, 3, **f32), ws=torch.empty(ws_bytes // 4, **f32),
                 order=torch.zeros(lib.geom_surface_order_words(B, nf, num, n_gt), **i32), loss=torch.empty((), **f32))
        wrote = ctypes.c_int(-1)
        tri = (nv, None, nf, None, None, None, None, None, None, None, None) if two_sided else \
              (nv, verts.data_ptr(), nf, faces.data_ptr(), order_tri.data_ptr(), o["tri_d"].data_ptr(), o["option"].data_ptr(),
               o["index"].data_ptr(), o["sq"].data_ptr(), o["closest"].data_ptr(), o["weights"].data_ptr())
        L.check(lib.geom_surface_scan_f32(B, n_gt, gt.data_ptr(), num, points.data_ptr(), o["sq_gt"].data_ptr(),
                                          o["idx_p"].data_ptr(), o["sq_pred"].data_ptr(), o["idx_g"].data_ptr(), *tri,
                                          u.data_ptr(), v.data_ptr(), coef_s, coef_o,
                                          o["order"].data_ptr() if with_records else None, flags, o["ws"].data_ptr(), ws_bytes,
                                          ctypes.byref(wrote), None, None, L.stream_ptr()), "geom_surface_scan_f32")
        assert wrote.value == int(with_records)
        other = o["sq_gt"] if two_sided else o["sq"]
        L.call("geom_surface_finalize_f32", B, nf, num, choices.data_ptr(), u.data_ptr(), v.data_ptr(), points.data_ptr(), n_gt,
               gt.data_ptr(), o["idx_g"].data_ptr(), o["idx_p"].data_ptr() if two_sided else None,
               None if two_sided else o["index"].data_ptr(), None if two_sided else o["closest"].data_ptr(),
               None if two_sided else o["weights"].data_ptr(), o["sq_pred"].data_ptr(), other.data_ptr(), coef_s, coef_o, coef_s,
               coef_o, 1, wrote.value, o["order"].data_ptr(), o["loss"].data_ptr())
        vf_ptr, vf_item = ops.vertex_faces(faces, nv)
        o["grad"] = torch.empty(B, nv, 3, **f32)
        L.call("geom_surface_gather_f32", B, nv, nf, vf_ptr.data_ptr(), vf_item.data_ptr(), num, n_gt, 1, o["order"].data_ptr(),
               None, o["grad"].data_ptr())
        return o

    a, c = run(True), run(False)
    for k in ("sq_gt", "idx_p", "sq_pred", "idx_g", "loss", "grad") + (() if two_sided else ("tri_d", "option", "index", "sq", "closest", "weights")):
        assert torch.equal(a[k], c[k]), k
    assert torch.equal(a["order"], c["order"])           # offsets, ordered ids AND records, word for word
    # the separate entry points
    d1, i1, d2, i2 = chamfer_nn(gt, points, flags)
    assert torch.equal(a["sq_gt"], d1) and torch.equal(a["idx_p"], i1) and torch.equal(a["sq_pred"], d2) and torch.equal(a["idx_g"], i2)
    if not two_sided:
        dt, pt, it = tri_distance_indexed(gt, verts, faces)
        assert torch.equal(a["tri_d"], dt) and torch.equal(a["option"], pt) and torch.equal(a["index"], it)
    # ... and the CPU oracle DIRECTLY on the launch the bench times, all 8 meshes of the shard: both Chamfer directions in
    # the launch's arithmetic (the reference's nnsearch restated; its FMA-contracted build for GEOM_FLAG_NN_FMA) and
    # the point-to-triangle scan (distance bits, region code, triangle index) -- not only through its HIP siblings
    import oracle
    gt_h, pts_h, verts_h = gt.cpu().numpy(), points.cpu().numpy(), verts.cpu().numpy()
    e1, j1, e2, j2 = oracle.chamfer_nn(gt_h, pts_h, oracle.FLAG_NN_FMA if fma else 0)
    assert np.array_equal(a["idx_p"].cpu().numpy(), j1) and np.array_equal(a["idx_g"].cpu().numpy(), j2)
    assert np.array_equal(a["sq_gt"].cpu().numpy().view(np.uint32), e1.view(np.uint32))
    assert np.array_equal(a["sq_pred"].cpu().numpy().view(np.uint32), e2.view(np.uint32))
    if not two_sided:
        et, ept, eit = oracle.tri_scan_indexed(gt_h, verts_h, Fc)
        assert np.array_equal(a["index"].cpu().numpy(), eit) and np.array_equal(a["option"].cpu().numpy(), ept)
        assert np.array_equal(a["tri_d"].cpu().numpy().view(np.uint32), et.view(np.uint32))


def test_prepare_launch_equals_draw_plus_prep(gpu):
    """geom_surface_prepare_f32 (draws + sampled points + the triangle records of the scan in ONE launch) against the
    separate draw launch and the scan's own prep launch: same random stream, same samples, and a loss / gradient that do
    not depend on which launch wrote the workspace."""
    V, Fc = meshgen.icosphere(4)
    B, num = 8, 3000
    verts = dev(meshgen.jittered_batch(V, B), gpu).requires_grad_(True)
    faces, gt = dev(Fc, gpu), dev(meshgen.gt_cloud(B, num), gpu)
    ops.manual_seed(31)
    a = ops.draw_samples(verts, faces, num, with_points=True)
    ops.manual_seed(31)
    b = ops.draw_samples(verts, faces, num, with_points=True, prepare_scan_for=num)
    assert len(b) == 5 and b[4] is not None
    for x, y in zip(a, b[:4]):
        assert torch.equal(x, y)
    res = []
    for tri_ws in (None, b[4]):
        verts.grad = None
        loss, sq_gt, sq_pred = ops.SurfaceLoss.apply(verts, faces, gt, b[0], b[1], b[2], False, 3000.0, b[3], tri_ws)
        loss.backward()
        res.append((loss.detach().clone(), sq_gt.clone(), sq_pred.clone(), verts.grad.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    # a single mesh does not take the fused route: draws only, no workspace
    c = ops.draw_samples(verts[:1].detach(), faces, num, with_points=True, prepare_scan_for=num)
    assert c[4] is None and c[3] is not None
    # and the whole helper still matches the CPU restatement through the prepared path
    ops.manual_seed(5)
    ch, u, v, pts, ws = ops.draw_samples(verts.detach(), faces, num, with_points=True, prepare_scan_for=num)
    loss = ops.SurfaceLoss.apply(verts.detach(), faces, gt, ch, u, v, False, 3000.0, pts, ws)[0]
    ref = ref_ops.point_to_surface(verts.detach().cpu()[:2], torch.from_numpy(Fc), gt.cpu()[:2], ch.cpu()[:2], u.cpu()[:2], v.cpu()[:2])
    part = ops.SurfaceLoss.apply(verts.detach()[:2].contiguous(), faces, gt[:2].contiguous(), ch[:2].contiguous(), u[:2].contiguous(),
                                 v[:2].contiguous(), False, 3000.0)[0]
    assert abs(part.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert torch.isfinite(loss)


def test_culled_chamfer_tiles_inside_the_surface_step(gpu):
    """The culled Chamfer tiles of the fused scan (ops.GtIndex handed to the loss) against the brute-force tiles ON THE SAME
    SAMPLES -- replayed through `draws=` -- : loss, both squared-distance outputs and the gradient bit for bit, in both
    arithmetics, with a Morton and with a deliberately incoherent gt order.  On this route the draw launch GENERATES the
    samples in visiting order (sorted uniforms from exponential spacings, csrc/draw_body.h): the position of a sample's face
    in the triangle order never decreases along the sample index, every face id is valid, and the sampled multiset is
    area-weighted like independent draws (frequencies against the areas; u = sqrt(U), v = U statistics)."""
    from geometrics_amd import chamfer_distance as cd
    from geometrics_amd.tri_distance import face_order
    V, Fc = meshgen.icosphere(4)
    B, num = 8, 3000
    verts = dev(meshgen.jittered_batch(V, B), gpu).requires_grad_(True)
    faces, gt = dev(Fc, gpu), dev(meshgen.gt_cloud(B, num), gpu)
    order = face_order(verts.detach(), faces).long()
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=gpu)
    gen = torch.Generator().manual_seed(3)
    shuffled = torch.stack([torch.randperm(num, generator=gen) for _ in range(B)]).to(torch.int32).to(gpu)
    try:
        for arithmetic in ("unfused", "fma"):
            cd.set_arithmetic(arithmetic)
            for gi in (ops.GtIndex(gt), ops.GtIndex(gt, shuffled)):
                ops.manual_seed(77)
                d = ops.draw_samples(verts, faces, num, with_points=True, prepare_scan_for=num, gt_index=gi)
                assert isinstance(d[4], ops.ScanPrep) and d[4].sample_index is not None
                choices, u, v, points = d[:4]
                assert int(choices.min()) >= 0 and int(choices.max()) < Fc.shape[0]
                pos = rank[choices]
                assert bool((pos[:, 1:] >= pos[:, :-1]).all())                   # generated in visiting order
                verts.grad = None
                loss, sq_gt, sq_pred = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, 3000.0, points, d[4], None, gi)
                loss.backward()
                culled = (loss.detach().clone(), sq_gt.clone(), sq_pred.clone(), verts.grad.clone())
                verts.grad = None                                                  # the same samples through the brute-force tiles
                loss, sq_gt, sq_pred = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, 3000.0)
                loss.backward()
                for x, y in zip(culled, (loss.detach(), sq_gt, sq_pred, verts.grad)):
                    assert torch.equal(x, y)
    finally:
        cd.set_arithmetic("unfused")
    # the sorted generation draws what independent draws would: area-weighted faces, u = sqrt(U1), v = U2
    gi = ops.GtIndex(gt)
    counts = torch.zeros(Fc.shape[0], dtype=torch.float64, device=gpu)
    us, vs = [], []
    ops.manual_seed(11)
    rounds = 40
    for _ in range(rounds):
        d = ops.draw_samples(verts.detach(), faces, num, with_points=True, prepare_scan_for=num, gt_index=gi)
        counts += torch.bincount(d[0][0], minlength=Fc.shape[0]).double()
        us.append(d[1][0]), vs.append(d[2][0])
    areas = ops.face_areas(verts.detach(), faces)[0].double()
    freq, p = counts / (rounds * num), areas / areas.sum()
    assert float((freq - p).abs().max()) < 6 * float((p.max() / (rounds * num)).sqrt())     # 6 sigma of a binomial frequency
    uu, vv = torch.cat(us), torch.cat(vs)
    assert abs(float((uu * uu).mean()) - 0.5) < 5e-3 and abs(float(vv.mean()) - 0.5) < 5e-3
    # the helper the training loop calls; an index built for another tensor is refused
    info = {"faces": faces}
    assert utils.batch_point_to_surface(verts.detach(), info, gt, num=num, gt_index=gi).isfinite()
    with pytest.raises(RuntimeError):
        utils.batch_point_to_surface(verts.detach(), info, gt.clone(), num=num, gt_index=gi)


@pytest.mark.parametrize("level,B,num,n_gt,sorted_route", [(2, 32, 64, 512, True), (3, 6, 1000, 2750, True), (4, 2, 4095, 8200, True),
                                                          (2, 7, 1531, 2466, True), (2, 80, 64, 256, True), (3, 6, 4096, 2750, False), (2, 40, 63, 448, False),
                                                          (2, 2, 500, 500, False)])
def test_sorted_draws_at_ragged_sizes(gpu, level, B, num, n_gt, sorted_route):
    """The visiting-order generation at the ends of its range (64 <= num < 4096 samples, and a step large enough for the
    fused scan route: >= 256 query tiles; outside, the draw launch falls back to independent draws and the scan to
    brute-force Chamfer tiles), small meshes, gt clouds of another size than the sample count, more meshes than the scan
    launch takes finalize roles for (64):
    samples in visiting order, every face valid, and loss / distances / gradient bit-identical to the brute-force tiles on
    the same samples."""
    from geometrics_amd.tri_distance import face_order
    V, Fc = meshgen.icosphere(level)
    verts = dev(meshgen.jittered_batch(V, B), gpu).requires_grad_(True)
    faces, gt = dev(Fc, gpu), dev(meshgen.gt_cloud(B, n_gt), gpu)
    gi = ops.GtIndex(gt)
    ops.manual_seed(5 + num)
    d = ops.draw_samples(verts, faces, num, with_points=True, prepare_scan_for=n_gt, gt_index=gi)
    choices, u, v, points = d[:4]
    assert isinstance(d[4], ops.ScanPrep) == sorted_route
    assert int(choices.min()) >= 0 and int(choices.max()) < Fc.shape[0]
    assert float(u.min()) >= 0 and float(u.max()) <= 1 and float(v.min()) >= 0 and float(v.max()) < 1
    if sorted_route:
        order = face_order(verts.detach(), faces).long()
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel(), device=gpu)
        pos = rank[choices]
        assert bool((pos[:, 1:] >= pos[:, :-1]).all())
    loss, sq_gt, sq_pred = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, 3000.0, points, d[4], None, gi)
    loss.backward()
    first = (loss.detach().clone(), sq_gt.clone(), sq_pred.clone(), verts.grad.clone())
    verts.grad = None
    loss, sq_gt, sq_pred = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, 3000.0)
    loss.backward()
    for x, y in zip(first, (loss.detach(), sq_gt, sq_pred, verts.grad)):
        assert torch.equal(x, y)
    ops.manual_seed(0, gpu)


def test_sorted_draws_are_shard_invariant(gpu):
    """The samples the culled route generates (in face-visiting order) for a mesh depend on the seed, the stream position,
    the mesh's GLOBAL index and its positions only -- not on which other meshes share the launch: 16 meshes drawn at once
    equal the same 16 drawn as two shards of 8 (mesh_offset 0 / 8), provided both derive the faces' visiting order from the
    same positions (the order is cached per face list on first use)."""
    from geometrics_amd.tri_distance import face_order
    V, Fc = meshgen.icosphere(4)
    faces = dev(Fc, gpu)
    face_order(dev(V, gpu).unsqueeze(0), faces)                       # the template: what every rank holds
    verts = dev(meshgen.jittered_batch(V, 16), gpu)
    gt = dev(meshgen.gt_cloud(16, 3000), gpu)

    def draw(v, g, first):
        ops.manual_seed(3041, gpu, mesh_offset=first)
        d = ops.draw_samples(v, faces, 3000, with_points=True, prepare_scan_for=3000, gt_index=ops.GtIndex(g))
        assert isinstance(d[4], ops.ScanPrep)
        return [t.clone() for t in d[:4]]

    whole = draw(verts, gt, 0)
    parts = [draw(verts[:8].contiguous(), gt[:8].contiguous(), 0), draw(verts[8:].contiguous(), gt[8:].contiguous(), 8)]
    for k in range(4):
        assert torch.equal(whole[k], torch.cat([parts[0][k], parts[1][k]]))
    ops.manual_seed(0, gpu)


def test_tri_surface_fused_call_equals_scan_plus_point_to_triangle(gpu):
    """geom_tri_surface_fwd_f32 (scan epilogue writes sqdist / closest / weights) against the two separate entry
    points, for the two-level scan (fused), the flat scan, the brute-force scan and a single mesh (split query tiles:
    the epilogue is replaced by the separate kernel) -- bitwise."""
    from geometrics_amd import _lib as L
    from geometrics_amd.tri_distance import face_order
    V, Fc = meshgen.icosphere(3)
    faces = dev(Fc, gpu)
    for B, n in ((3, 700), (1, 300)):
        verts, pts = dev(meshgen.jittered_batch(V, B), gpu), dev(meshgen.gt_cloud(B, n), gpu)
        order = face_order(verts, faces)
        ws_bytes = L.lib().geom_tri_distance_workspace_bytes(B, n, Fc.shape[0])
        ws = torch.empty(ws_bytes // 4 + 4, device=gpu)
        f32 = dict(dtype=torch.float32, device=gpu)
        i32 = dict(dtype=torch.int32, device=gpu)
        d0, p0, i0 = torch.empty(B, n, **f32), torch.empty(B, n, **i32), torch.empty(B, n, **i32)
        L.check(L.lib().geom_tri_distance_indexed_ws_f32(B, n, pts.data_ptr(), V.shape[0], verts.data_ptr(), Fc.shape[0],
                                                         faces.data_ptr(), order.data_ptr(), d0.data_ptr(), p0.data_ptr(),
                                                         i0.data_ptr(), 0, ws.data_ptr(), ws_bytes, L.stream_ptr()), "scan")
        s0, c0, w0 = torch.empty(B, n, **f32), torch.empty(B, n, 3, **f32), torch.empty(B, n, 3, **f32)
        L.call("geom_p2tri_loss_fwd_f32", B, n, pts.data_ptr(), V.shape[0], verts.data_ptr(), Fc.shape[0], faces.data_ptr(),
               p0.data_ptr(), i0.data_ptr(), s0.data_ptr(), c0.data_ptr(), w0.data_ptr())
        for order_ptr, flags in ((order.data_ptr(), 0), (None, 0), (order.data_ptr(), 4)):
            d, p, i = torch.empty(B, n, **f32), torch.empty(B, n, **i32), torch.empty(B, n, **i32)
            s, c, w = torch.empty(B, n, **f32), torch.empty(B, n, 3, **f32), torch.empty(B, n, 3, **f32)
            L.check(L.lib().geom_tri_surface_fwd_f32(B, n, pts.data_ptr(), V.shape[0], verts.data_ptr(), Fc.shape[0],
                                                     faces.data_ptr(), order_ptr, d.data_ptr(), p.data_ptr(), i.data_ptr(),
                                                     s.data_ptr(), c.data_ptr(), w.data_ptr(), flags, ws.data_ptr(), ws_bytes,
                                                     L.stream_ptr()), "fused")
            for got, want in ((d, d0), (p, p0), (i, i0), (s, s0), (c, c0), (w, w0)):
                assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("culled", [False, True])
def test_finalize_tail_of_the_scan_launch_equals_the_separate_launch(gpu, culled):
    """ops.scan_finalize_tail: the loss sum and the face ordering of the points done by trailing workgroups of the fused scan
    launch (each mesh as soon as its triangle tiles are through) against geom_surface_finalize_f32 in a launch of its own:
    loss, both distance outputs and the vertex gradient bit for bit -- with a gradient (ordering + loss roles), without one
    (loss role only), repeated on the same workspace (the completion counters reset themselves), and as a replayed HIP graph."""
    V, Fc = meshgen.icosphere(4)
    B, num = 8, 3000
    verts = dev(meshgen.jittered_batch(V, B), gpu).requires_grad_(True)
    faces, gt = dev(Fc, gpu), dev(meshgen.gt_cloud(B, num), gpu)
    gi = ops.GtIndex(gt) if culled else None
    info = {"faces": faces}

    def run(tail, grad=True, seed=21):
        ops.scan_finalize_tail = tail
        try:
            ops.manual_seed(seed)
            verts.grad = None
            if grad:
                loss = utils.batch_point_to_surface(verts, info, gt, num=num, gt_index=gi)
                loss.backward()
                return loss.detach().clone(), verts.grad.clone()
            with torch.no_grad():
                return utils.batch_point_to_surface(verts, info, gt, num=num, gt_index=gi).clone(), None
        finally:
            ops.scan_finalize_tail = True

    for seed in (21, 22, 23):
        a, b = run(True, seed=seed), run(False, seed=seed)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = run(True, grad=False), run(False, grad=False)
    assert torch.equal(a[0], b[0])
    # captured: the trailing workgroups spin inside the replayed launch exactly as in the eager one
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    ops.manual_seed(31)
    verts.grad = None
    with torch.cuda.graph(g):
        loss = utils.batch_point_to_surface(verts, info, gt, num=num, gt_index=gi)
        loss.backward()
    want = None
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        got = (loss.detach().clone(), verts.grad.clone())
        if want is None:
            want = got
    assert bool(torch.isfinite(want[0])) and bool(torch.isfinite(want[1]).all())
    ops.manual_seed(0, gpu)


def test_finalize_roles_give_up_instead_of_hanging(gpu):
    """A role workgroup of the fused scan launch waits on a completion counter; if the count can never be reached (here: a
    counter knocked 100 below zero between the prepare launch and the scan) it gives up after ~2 M polls: the launch's loss
    comes out as NaN, the role reads nothing of the incomplete results and marks its status word, and the BACKWARD writes
    NaN for that mesh's vertices -- never a walk through a half-built order -- while the meshes whose roles got through keep
    the gradient the separate launch gives, bit for bit.  The device is not hung; the next forward notices the status
    (no synchronisation: a pinned copy) and switches the roles off for the rest of the process, with a warning; results
    from then on are the separate launch's."""
    import time
    import warnings
    from geometrics_amd import _lib
    V, Fc = meshgen.icosphere(4)
    B, num = 8, 3000
    verts = dev(meshgen.jittered_batch(V, B), gpu).requires_grad_(True)
    faces, gt = dev(Fc, gpu), dev(meshgen.gt_cloud(B, num), gpu)
    gi = ops.GtIndex(gt)
    off = _lib.lib().geom_surface_tail_counters_offset(B, num, Fc.shape[0])
    assert off > 0 and off % 4 == 0
    assert ops.scan_finalize_tail and not ops.finalize_roles_gave_up()
    try:
        ops.manual_seed(9)
        d = ops.draw_samples(verts, faces, num, with_points=True, prepare_scan_for=num, gt_index=gi)
        assert isinstance(d[4], ops.ScanPrep)
        counters = d[4].tri_ws.view(torch.int32)[off // 4:]
        assert int(counters[::32][:2 * B + 1].abs().sum()) == 0          # zeroed by the prepare launch
        counters[3 * 32] = -100                                          # mesh 3's triangle tiles can never reach their count
        torch.cuda.synchronize()
        t0 = time.time()
        loss, _, _ = ops.SurfaceLoss.apply(verts, faces, gt, d[0], d[1], d[2], False, 3000.0, d[3], d[4], None, gi)
        assert bool(torch.isnan(loss))                                   # said loudly
        assert time.time() - t0 < 60
        loss.backward(torch.ones((), device=gpu))                        # (a finite seed: the NaN below is the kernel's own)
        g = verts.grad.clone()
        assert bool(torch.isnan(g).all())                                # the loss role gave up as well: every mesh is NaN, none is garbage
        torch.cuda.synchronize()
        # the next forward sees the status words of the last one and falls back to the separate finalize launch
        verts.grad = None
        ops.manual_seed(9)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            after = utils.batch_point_to_surface(verts, {"faces": faces}, gt, num=num, gt_index=gi)
            after.backward()
        assert bool(torch.isfinite(after)) and bool(torch.isfinite(verts.grad).all())
        assert ops.finalize_roles_gave_up() and not ops.scan_finalize_tail
        assert any("gave up" in str(w.message) for w in caught)
        # ... with the results of the separate launch (= of the roles when they get through: tested above)
        verts.grad = None
        ops.manual_seed(9)
        again = utils.batch_point_to_surface(verts, {"faces": faces}, gt, num=num, gt_index=gi)
        assert torch.equal(again, after)
    finally:
        ops.scan_finalize_tail = True
        ops._roles_gave_up = False
        ops._roles_watch.clear()
        ops.manual_seed(0, gpu)


def test_the_timed_route_against_the_oracle_at_the_config5_shard(gpu):
    """What bench.py times, checked DIRECTLY (round-4 review: the route was only compared with the brute-force tiles on the
    same samples, and those with the oracle on other draws): BASELINE config 5's shard -- 8 meshes, 2562 vertices / 5120
    faces, 3000 + 3000 points -- with the samples the visiting-order generator emits under a gt index (k-d orders, as the
    bench builds them), the culled Chamfer tiles and the finalize pass inside the scan launch.  The (choices, u, v) it drew
    go through the CPU restatement of the reference (oracle.ref_ops.point_to_surface, utils.py:441-502, arg-min stages from
    the C oracle): NN indices of both directions and the winning triangle + its region code bit-exact, the arg-min
    distances bit for bit, the loss within 1e-5, the gradient row by row against the float64 closed form."""
    import oracle
    from geometrics_amd.tri_distance import kd_order
    V, Fc = meshgen.icosphere(4)
    B, num = 8, 3000
    verts_np, gt_np = meshgen.jittered_batch(V, B), meshgen.gt_cloud(B, num)
    verts = dev(verts_np, gpu).requires_grad_(True)
    faces, gt = dev(Fc, gpu), dev(gt_np, gpu)
    gi = ops.GtIndex(gt, torch.stack([kd_order(gt[i]) for i in range(B)]))
    assert ops.scan_finalize_tail
    ops.manual_seed(2041)
    choices, u, v, points, prep = ops.draw_samples(verts, faces, num, with_points=True, prepare_scan_for=num, gt_index=gi)
    assert isinstance(prep, ops.ScanPrep) and prep.sample_index is not None          # the culled route is what runs
    seen = {}
    ops.scan_capture = seen
    try:
        loss, sq_gt, sq_pred = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, 3000.0, points, prep, None, gi)
    finally:
        ops.scan_capture = None
    loss.backward()
    ch, uu, vv = (t.cpu().numpy() for t in (choices, u, v))
    # the sampled points themselves: bitwise the reference's barycentric combination of the drawn corners
    pred = ref_ops.sample_points(torch.from_numpy(verts_np), torch.from_numpy(Fc), torch.from_numpy(ch), torch.from_numpy(uu),
                                 torch.from_numpy(vv)).numpy()
    assert np.array_equal(bits(points.cpu().numpy()), bits(pred))
    d_gt, i_gt, d_pred, i_pred = oracle.chamfer_nn(gt_np, pred)
    assert np.array_equal(seen["idx_gt"].cpu().numpy(), i_gt) and np.array_equal(seen["idx_pred"].cpu().numpy(), i_pred)
    assert np.array_equal(bits(sq_pred.cpu().numpy()), bits(d_pred))
    t_d, t_opt, t_idx = oracle.tri_scan_indexed(gt_np, verts_np, Fc)
    assert np.array_equal(seen["tri_index"].cpu().numpy(), t_idx) and np.array_equal(seen["tri_option"].cpu().numpy(), t_opt)
    assert np.array_equal(bits(seen["tri_dist"].cpu().numpy()), bits(t_d))
    cv = torch.from_numpy(verts_np).requires_grad_(True)
    ref = ref_ops.point_to_surface(cv, torch.from_numpy(Fc), torch.from_numpy(gt_np), torch.from_numpy(ch), torch.from_numpy(uu),
                                   torch.from_numpy(vv))
    close(loss.item(), ref.item(), 1e-5)
    exact_loss, exact, mass, floor = fp64_surface_gradient(verts_np, Fc, gt_np, ch, uu, vv, two_sided=False)
    close(loss.item(), exact_loss, 1e-5)
    rows_close(verts.grad.cpu().numpy(), exact, mass, ROW_RTOL_SURFACE, "timed route, grad_verts at the config-5 shard", floor,
               ROW_FLOOR_ULPS)


def test_fan_out_sums_its_handles_gradients_in_one_launch(gpu):
    """utils.fan_out(x, n): n handles on one tensor whose gradients meet in ONE launch (geom_sum_tensors_f32: ((g0 + g1) + g2) + ...)
    -- the same values as using x n times (autograd's pairwise accumulation in the same order gives the same bits for three
    handles; for more the order of autograd's adds is its own, so the comparison is to fp32 round-off)."""
    torch.manual_seed(15)
    x = torch.randn(16, 482, 3, device=gpu, requires_grad=True)
    ws = [torch.randn(16, 482, 3, device=gpu) for _ in range(6)]
    hs = utils.fan_out(x, 6)
    assert all(h.data_ptr() == x.data_ptr() for h in hs) and len({id(h) for h in hs}) == 6
    sum((h * w).sum() for h, w in zip(hs, ws)).backward()
    expect = ((((ws[0] + ws[1]) + ws[2]) + ws[3]) + ws[4]) + ws[5]
    assert torch.equal(x.grad, expect)
    y = x.detach().clone().requires_grad_(True)
    sum((y * w).sum() for w in ws).backward()
    assert float((x.grad - y.grad).abs().max()) <= 1e-6 * float(y.grad.abs().max())
    a, = utils.fan_out(x, 1)
    assert a is x
    hs = utils.fan_out(x, 3)                      # a handle nobody uses contributes nothing
    x.grad = None
    ((hs[0] * ws[0]).sum() + (hs[2] * ws[2]).sum()).backward()
    assert torch.equal(x.grad, ws[0] + ws[2])
    # a gradient that arrives as a column slice of a wider buffer (the coordinates' share of a block's 1155-wide input gradient)
    # is read in place (geom_sum_tensors_rows_f32): same sum
    wide = torch.randn(16, 482, 1155, device=gpu)
    hs = utils.fan_out(x, 3)
    x.grad = None
    torch.autograd.backward(hs, [ws[0], wide[..., :3], ws[1]])
    assert torch.equal(x.grad, (ws[0] + wide[..., :3]) + ws[1])


def test_sum_losses_is_one_launch_and_the_same_sum(gpu):
    torch.manual_seed(16)
    ts = [torch.randn((), device=gpu, requires_grad=True) for _ in range(6)]
    total = utils.sum_losses(*ts)
    expect = ((((ts[0] + ts[1]) + ts[2]) + ts[3]) + ts[4]) + ts[5]
    assert torch.equal(total.detach(), expect.detach())
    (total * 3.0).backward()
    assert all(float(t.grad) == 3.0 for t in ts)
    assert utils.sum_losses(ts[0]) is ts[0]
