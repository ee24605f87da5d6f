"""-m gpu: NaN and Inf through the layer kernels, as torch carries them ("Non-finite values").

A few planted values -- one NaN, one +Inf, one -Inf, or +Inf and -Inf in the same column of two neighbours of one vertex, whose
aggregate is NaN while both sources are Inf -- in an aggregated column or a pass-through one, at an ordinary vertex, at a pole
of the 482-vertex template (33-entry row: table + CSR tail) or in the last row of the last mesh (ragged last row tile); every
other value is N(0, 1), so fp32 overflows nowhere float64 does not and the KIND of every sum is independent of its order.

The float64 references aggregate over a row's stored entries (ref_ops.sparse_aggregate): a non-finite value reaches exactly the
rows that hold its vertex -- the reference's dense product, where 0 * NaN is NaN, poisons a superset
(tests/test_nonfinite_host.py).  helpers.nonfinite_close: the finite masks agree at every element, then (kinds=True) NaN, +Inf
and -Inf agree, then the finite elements are within the bound the finite test of the same kernel uses."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from geometrics_amd import _lib as L
from geometrics_amd import layers, meshgen, utils
from helpers import BN_MAX_KNIFE, finite_part, golden, nonfinite_close, vertex_bn64
from oracle import ref_ops

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
EPS32 = 2.0 ** -24
# a row's sum: at most 33 terms on the meshes, 37 on the random graph (asserted), + the bias, + the project's allowance of 8 for
# the products and the activation around it (helpers.BN_ROW_RTOL is built the same way)
AGG_RTOL = (38 + 8) * EPS32
BIAS_RTOL = 1e-6                     # the bias gradient's bound in tests/test_aggregate_kernels_gpu.py
VALUES = ("nan", "+inf", "-inf", "pair")
ACT64 = {0: lambda t: t, 1: torch.relu, 2: F.elu}


# ---- meshes and planted values -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes(gpu):
    """name -> (batch, CSR with its tables, the float64 adjacency on the host, [(location, vertex)])."""
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    g = torch.Generator(device="cpu").manual_seed(48)
    dense = (torch.rand(48, 48, generator=g) < 0.5).float()
    dense.fill_diagonal_(1.0)
    out = {}
    for name, adj, batch in (("ico162", utils.adj_init(to(meshgen.icosphere(2)[1]))["adj"], 3),
                             ("template482", utils.adj_init(to(golden("adj_482")["faces"]))["adj"], 2),
                             ("random48", dense.to(gpu), 2)):
        csr, a64 = layers.adjacency_csr(adj), adj.double().cpu()
        lens = (a64 != 0).sum(1)
        assert int(lens.max()) <= 37
        where = [("ordinary", csr.nv // 3), ("last", csr.nv - 1)]
        if name == "template482":
            assert int(lens.max()) == 33 and csr.over is not None and int(lens[csr.nv // 3]) <= 8
            where.insert(1, ("pole", int(lens.argmax())))
        out[name] = (batch, csr, a64, where)
    assert out["ico162"][1].ell_w == 8 and out["ico162"][1].over is None and out["random48"][1].ell_w == 0
    assert (3 * 162) % 64 and (3 * 162) % 16                   # 486 rows: the last row tile is ragged
    return out


def plants(mesh, columns, values=VALUES):
    """(label, [(mesh, vertex, column, value)]) of every combination of value, column and location on `mesh`: `last` in the last
    mesh, the others in the first.  pair: +Inf and -Inf at the first two neighbours of the location's vertex."""
    batch, _, a64, where = mesh
    for value, (cname, col), (lname, v) in itertools.product(values, columns, where):
        b = batch - 1 if lname == "last" else 0
        if value == "pair":
            n1, n2 = [int(u) for u in a64[v].nonzero().flatten().tolist() if u != v][:2]
            cells = [(b, n1, col, INF), (b, n2, col, -INF)]
        else:
            cells = [(b, v, col, {"nan": NAN, "+inf": INF, "-inf": -INF}[value])]
        yield "%s, %s column %d, %s vertex %d" % (value, cname, col, lname, v), cells


def planted(t, cells):
    t = t.clone()
    for b, v, col, value in cells:
        t[b, v, col] = value
    return t


def _aggregate64(a64, s, k):
    return torch.cat((ref_ops.sparse_aggregate(a64, s[..., :k]), s[..., k:]), dim=-1)


def forward64(a64, sup, bias, k, act):
    """(act([A . S[..., :k] | S[..., k:]] + bias), its mass) in float64 over the rows' stored entries."""
    s = sup.double().cpu()
    b64 = torch.zeros(s.shape[-1], dtype=torch.float64) if bias is None else bias.double().cpu()
    return ACT64[act](_aggregate64(a64, s, k) + b64), _aggregate64(a64.abs(), finite_part(s).abs(), k) + b64.abs()


def with_derivative64(gout, saved, act):
    """g' = g * act'(saved).  ReLU: torch's threshold_backward, out <= 0 ? 0 : g -- a NaN output lets g through.  ELU:
    out > 0 ? g : g * (out + 1) -- a NaN output gives NaN (torch's own kernels answer g or NaN there, depending on the device
    and, on the host, on whether the element falls into a vector lane or the scalar tail: DESIGN.md states the package's rule)."""
    g = gout.double().cpu()
    if act == 0:
        return g
    out = saved.double().cpu()
    if act == 1:
        return torch.where(out <= 0, torch.zeros_like(g), g)
    return torch.where(out > 0, g, g * (out + 1))


class _Elu64(torch.autograd.Function):
    """F.elu for the float64 references under autograd, its derivative written out as with_derivative64 states it."""

    @staticmethod
    def forward(ctx, x):
        out = F.elu(x)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        return with_derivative64(g, ctx.saved_tensors[0], 2)


def backward64(a64, gp, k):
    """([A^T . g'[..., :k] | g'[..., k:]], column sums of g') and their masses."""
    m = finite_part(gp).abs()
    at = a64.t().contiguous()
    c = gp.shape[-1]
    return (_aggregate64(at, gp, k), _aggregate64(at.abs(), m, k)), (gp.reshape(-1, c).sum(0), m.reshape(-1, c).sum(0))


# ---- a. the aggregation entry points ----------------------------------------------------------------------------------------------
SHAPES_A = [(72, 24), (120, 12), (52, 6), (7, 3)]          # the table's split-3 and split-10 kernels, any width at VEC 4, at VEC 1


def _table(csr, transposed):
    col, val, over = (csr.ell_col_t, csr.ell_val_t, csr.over_t) if transposed else (csr.ell_col, csr.ell_val, csr.over)
    return (csr.ell_w, col, val) + tuple(over or (None, None, None))


def _operands(batch, nv, c, gpu, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(*s, generator=g).to(gpu) for s in ((batch, nv, c), (c,), (batch, nv, c))]


def _forward_kernels(csr, sup, bias, k, act):
    """{entry point: output} of the CSR kernel and, where the adjacency has a table, the table kernel."""
    b, nv, c = sup.shape
    out = {"csr": torch.full_like(sup, 7.0)}
    L.call("geom_zn_gcn_aggregate_fwd_f32", b, nv, c, k, csr.rowptr, csr.col, csr.val, sup, bias, act, out["csr"])
    if csr.ell_w:
        out["table"] = torch.full_like(sup, 7.0)
        L.call("geom_zn_gcn_aggregate_ell_fwd_f32", b, nv, c, k, *_table(csr, False), sup, bias, act, out["table"], None)
    return out


def _backward_kernels(csr, gout, saved, k, act):
    """{entry point: (input gradient, bias gradient)}."""
    b, nv, c = gout.shape
    words = L.lib().geom_zn_gcn_bwd_scratch_floats(b, nv, c)
    new = lambda: (torch.full_like(gout, 7.0), torch.full((c,), 7.0, device=gout.device), torch.empty(words, device=gout.device))
    out = {"csr": new()}
    L.call("geom_zn_gcn_aggregate_bwd_f32", b, nv, c, k, csr.rowptr_t, csr.col_t, csr.val_t, gout, saved, act, *out["csr"])
    if csr.ell_w:
        out["table"] = new()
        L.call("geom_zn_gcn_aggregate_ell_bwd_f32", b, nv, c, k, *_table(csr, True), gout, saved, None, act, *out["table"])
    return {name: t[:2] for name, t in out.items()}


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "relu", "elu"])
@pytest.mark.parametrize("c,k", SHAPES_A, ids=["%d-%d" % s for s in SHAPES_A])
@pytest.mark.parametrize("name", ["ico162", "template482", "random48"])
def test_aggregation_entry_points_carry_planted_values_as_the_sparse_float64_sum(gpu, meshes, name, c, k, act):
    """geom_zn_gcn_aggregate_{fwd,bwd}_f32 and the table entry points: values planted in `support` (forward), in the upstream
    gradient and in the saved output (backward).  Pins the padded table slots (a NaN of the row's own element, which a padded
    slot loads, must not reach the sum), the CSR tail and all three activations with their derivatives."""
    mesh = meshes[name]
    batch, csr, a64, _ = mesh
    sup, bias, gout = _operands(batch, csr.nv, c, gpu, 100 * c + act)
    saved = ACT64[act](torch.randn(batch, csr.nv, c, generator=torch.Generator(device="cpu").manual_seed(c)).to(gpu))
    cases = 0
    for label, cells in plants(mesh, (("aggregated", k - 1), ("pass-through", k))):
        want, mass = forward64(a64, planted(sup, cells), bias, k, act)
        assert bool(torch.isfinite(want).any()) and (act or not bool(torch.isfinite(want).all()))      # (relu(-Inf) is 0, elu(-Inf) -1)
        for kernel, got in _forward_kernels(csr, planted(sup, cells), bias, k, act).items():
            nonfinite_close(got, want, mass, AGG_RTOL, "%s forward, %s" % (kernel, label))
        for operand in ("gradient", "saved output") if act else ("gradient",):
            g = planted(gout, cells) if operand == "gradient" else gout
            o = planted(saved, cells) if operand == "saved output" else saved
            gp = with_derivative64(g, o, act)
            (want, mass), (want_b, mass_b) = backward64(a64, gp, k)
            for kernel, (grad, gb) in _backward_kernels(csr, g, o if act else None, k, act).items():
                what = "%s backward, %s in the %s" % (kernel, label, operand)
                nonfinite_close(grad, want, mass, AGG_RTOL, what)
                nonfinite_close(gb, want_b, mass_b, BIAS_RTOL, what + " (bias gradient)")
            cases += 1
    assert cases == len(VALUES) * 2 * len(mesh[3]) * (2 if act else 1)


@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
@pytest.mark.parametrize("name", ["ico162", "template482"])
def test_head_and_narrow_head_entry_points_carry_planted_values(gpu, meshes, name, act):
    """The head (positions = base + scale * out[..., :3] out of the aggregation launch) and the narrow head (column group 0
    alone) at 192 / 64: values planted in `support` (forward; the ReLU's sign words then hold a set bit for a NaN output) and in
    grad_pos (backward, whose relu' comes from those sign words: the derivative is taken at the kernels' own fp32 output)."""
    mesh = meshes[name]
    batch, csr, a64, _ = mesh
    nv, c, k, scale, w = csr.nv, 192, 64, 0.01, csr.ell_w
    sup0, bias, _ = _operands(batch, nv, c, gpu, 7 + act)
    g = torch.Generator(device="cpu").manual_seed(8)
    base, grad_pos0 = torch.randn(batch, nv, 3, generator=g).to(gpu), torch.randn(batch, nv, 3, generator=g).to(gpu)
    rows_wide = int(L.lib().geom_zn_gcn_bwd_partial_rows(batch, nv, c, k, w))
    for label, cells in plants(mesh, (("position", 1), ("aggregated", k - 1), ("pass-through", k))):
        sup = planted(sup0, cells)
        want, mass = forward64(a64, sup, bias, k, act)
        want_pos, mass_pos = base.double().cpu() + scale * want[..., :3], base.double().cpu().abs() + scale * mass[..., :3]
        out, pos, narrow = torch.full_like(sup, 7.0), torch.full_like(base, 7.0), torch.full_like(base, 7.0)
        mask = torch.zeros(L.lib().geom_zn_gcn_relu_mask_words(batch, nv, c, k), dtype=torch.int16, device=gpu) if act else None
        sign = torch.zeros(batch * nv, dtype=torch.int16, device=gpu) if act else None
        L.call("geom_zn_gcn_aggregate_ell_head_fwd_f32", batch, nv, c, k, *_table(csr, False), sup, bias, act, out, mask, base, scale, pos)
        L.call("geom_zn_gcn_narrow_head_fwd_f32", batch, nv, c, k, *_table(csr, False), sup, bias, act, base, scale, narrow, sign)
        nonfinite_close(out, want, mass, AGG_RTOL, "head forward, " + label)
        nonfinite_close(pos, want_pos, mass_pos, AGG_RTOL, "head positions, " + label)
        nonfinite_close(narrow, want_pos, mass_pos, AGG_RTOL, "narrow head positions, " + label)
        # backward: [scale * grad_pos | 0] through relu' at the kernel's own output, grad_pos planted where a position column is
        col = cells[0][2]
        grad_pos = planted(grad_pos0, [(b, v, col, value) for b, v, _, value in cells]) if col < 3 else grad_pos0
        gout = torch.zeros(batch, nv, c, dtype=torch.float64)
        gout[..., :3] = scale * grad_pos.double().cpu()
        (want_g, mass_g), (want_b, mass_b) = backward64(a64, with_derivative64(gout, out, act), k)
        words = L.lib().geom_zn_gcn_bwd_scratch_floats(batch, nv, c)
        grad, gb, scr = torch.full_like(sup, 7.0), torch.full((c,), 7.0, device=gpu), torch.empty(words, device=gpu)
        L.call("geom_zn_gcn_aggregate_ell_head_bwd_f32", batch, nv, c, k, *_table(csr, True), grad_pos, scale, mask, act, grad, gb, scr)
        nonfinite_close(grad, want_g, mass_g, AGG_RTOL, "head backward, " + label)
        nonfinite_close(gb, want_b, mass_b, BIAS_RTOL, "head backward (bias gradient), " + label)
        gs4, part = torch.full((batch * nv, 4), 7.0, device=gpu), torch.full((rows_wide, c), 7.0, device=gpu)
        L.call("geom_zn_gcn_narrow_head_bwd_f32", batch, nv, c, k, *_table(csr, True), grad_pos, scale, sign, act, gs4, part)
        nonfinite_close(gs4.view(batch, nv, 4), want_g[..., :4], mass_g[..., :4], AGG_RTOL, "narrow head backward, " + label)
        nonfinite_close(part.double().sum(0), want_b, mass_b, BIAS_RTOL, "narrow head backward (bias gradient), " + label)


# ---- c. VertexBatchNorm on the C ABI -------------------------------------------------------------------------------------------------
BN_NV, BN_EPS, BN_MOMENTUM, BN_SCALE = 7, 1e-5, 0.1, 0.5
BN_SHAPES = [(4, 36), (21, 192)]                 # the float4 kernels, the scalar kernels (tests/test_vertex_bn_gpu.py TABLE)


def _bn_device(gpu, x, gamma, beta, old, relu, res, training, g):
    """geom_vertex_bn_fwd_f32 (+ _bwd_f32 in training mode) -> {output: tensor}."""
    b, nv, c = x.shape
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)
    xd, rm, rv = dev(x), dev(old[0]), dev(old[1])
    out, mean, invstd = torch.full_like(xd, 7.0), torch.full((nv,), 7.0, device=gpu), torch.full((nv,), 7.0, device=gpu)
    L.call("geom_vertex_bn_fwd_f32", b, nv, c, xd, dev(gamma), dev(beta), rm, rv, int(training), BN_MOMENTUM, BN_EPS, int(relu),
           dev(res), c, BN_SCALE, out, mean, invstd)
    got = {"out": out}
    if training:
        got.update(save_mean=mean, save_invstd=invstd, running_mean=rm, running_var=rv)
        gx, gr, gw, gb = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0), torch.full((nv,), 7.0, device=gpu), torch.full((nv,), 7.0, device=gpu)
        L.call("geom_vertex_bn_bwd_f32", b, nv, c, xd, dev(g), dev(gamma), dev(beta), mean, invstd, int(relu), int(res is not None),
               BN_SCALE, gx, gr if res is not None else None, gw, gb, None)
        got.update(grad_x=gx, grad_weight=gw, grad_bias=gb)
        if res is not None:
            got["grad_residual"] = gr
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
@pytest.mark.parametrize("res", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "identity"])
@pytest.mark.parametrize("b,c", BN_SHAPES, ids=["vec_4x36", "scalar_21x192"])
def test_vertex_batchnorm_kernels_carry_planted_values(gpu, b, c, relu, res, training):
    """geom_vertex_bn_fwd_f32 / _bwd_f32 against helpers.vertex_bn64, values planted in x, then in the upstream gradient.
    kinds=False: the variance of a row that holds an Inf is Inf - Inf; only the non-finite mask is determinate.  Training: the
    planted vertex is non-finite for every mesh and column (relu(NaN) is NaN), the other vertices keep their bounds."""
    rng = np.random.default_rng([1909, b, c])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    x0, r0, g0 = (f32(rng.standard_normal((b, BN_NV, c))) for _ in range(3))
    gamma, beta = f32(rng.uniform(0.5, 2.0, BN_NV)), f32(rng.uniform(-1.0, 1.0, BN_NV))
    old = (f32(0.5 * rng.standard_normal(BN_NV)), f32(rng.uniform(0.5, 1.5, BN_NV)))
    residual = r0 if res else None
    cells_of = {"nan": [(1, 2, 5, NAN)], "+inf": [(b - 1, BN_NV - 1, c - 1, INF)], "-inf": [(0, 0, 0, -INF)],
                "pair": [(0, 3, 1, INF), (b - 1, 3, c - 2, -INF)]}

    def reference(x, g):
        return vertex_bn64(x, gamma, beta, BN_EPS, relu, residual, BN_SCALE, g if training else None,
                           running=None if training else old, momentum=BN_MOMENTUM, old_running=old)
    # an element on the ReLU's kink may take either branch in fp32: no upstream gradient there, and its output is left out
    # (tests/test_vertex_bn_gpu.py does the same)
    knife = reference(x0, g0)[2]
    assert knife.mean() <= BN_MAX_KNIFE
    g0 = g0 * ~knife
    for value, operand in itertools.product(VALUES, ("x", "gradient") if training else ("x",)):
        x, g = x0.copy(), g0.copy()
        for i, v, col, what in cells_of[value]:
            (x if operand == "x" else g)[i, v, col] = what
        with np.errstate(all="ignore"):
            exact = reference(x, g)[0]
            mass = reference(finite_part(x), finite_part(g))[1]                  # every non-finite factor replaced by 0
        if "grad_residual" in exact:
            mass["grad_residual"] = np.abs(finite_part(g)) * BN_SCALE
        got = _bn_device(gpu, x, gamma, beta, old, relu, residual, training, g)
        seen = False
        for key, t in got.items():
            rtol = 0.0 if key == "grad_residual" else 8 * EPS32 if (key == "out" and not training) else (16 + 6 + 4 + 8) * EPS32
            pick = (~knife | ~np.isfinite(exact[key])) if key == "out" else Ellipsis
            nonfinite_close(t.cpu().numpy()[pick], exact[key][pick], mass[key][pick], rtol,
                            "vertex_bn %s, %s in %s" % (key, value, operand), kinds=False)
            seen = seen or not np.isfinite(exact[key]).all()
        # (nothing non-finite is left where eval's relu(-Inf) is 0, or where a planted gradient sits behind a closed ReLU)
        assert np.isfinite(exact["out"]).any() and (seen or (relu and (operand == "gradient" or value == "-inf")))
        if training and operand == "x":          # one statistic per vertex: every mesh and column of the planted vertex
            v = cells_of[value][0][1]
            assert not np.isfinite(exact["out"][:, v]).any() and np.isfinite(np.delete(exact["out"], v, axis=1)).all()


# ---- b. layers through every product route -------------------------------------------------------------------------------------------
ROW_RTOL_GEMM = 1.5e-6                       # tests/test_dense_gpu.py: a product's element against its product mass
LAYER_RTOL = ROW_RTOL_GEMM + AGG_RTOL        # a product, then a row's sum of its elements
ACTIVATIONS = {"relu": (F.relu, 1, torch.relu), "elu": (F.elu, 2, _Elu64.apply)}      # (the layers', the kernels' code, the float64 reference's)


def _layer_masses(a64, x, w, bias, split, out64, seed, act):
    """The |.|-chains of one layer's forward and backward with every non-finite factor replaced by 0: {output: mass}."""
    xf, wa = finite_part(x).abs(), w.abs()
    k = w.shape[-1] // split
    out_mass = _aggregate64(a64.abs(), xf @ wa, k) + bias.abs()
    gpm = finite_part(with_derivative64(seed, out64, act)).abs()
    if act == 2:
        # elu' = out + 1 = exp(pre) on the negative branch: the pre-activation's own rounding, rtol * its mass in ABSOLUTE terms,
        # is a RELATIVE error of that factor -- the term's mass grows by (1 + the forward mass)
        gpm = gpm * torch.where(out64 <= 0, 1 + out_mass, torch.ones_like(out_mass))
    dsm = _aggregate64(a64.t().contiguous().abs(), gpm, k)
    rows = lambda t: t.reshape(-1, t.shape[-1])
    return {"out": out_mass, "grad_x": dsm @ wa.t(), "grad_weight": rows(xf).t() @ rows(dsm), "grad_bias": rows(gpm).sum(0)}


def _layer_case(gpu, cls, b, cin, c, seed):
    """A layer of class `cls` with seeded parameters, its input and upstream gradient (unbatched for ZERON_GCN)."""
    torch.manual_seed(seed)
    layer = cls(cin, c).to(gpu)
    with torch.no_grad():
        layer.bias.uniform_(-0.5, 0.5)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    shape = (162, ) if cls is layers.ZERON_GCN else (b, 162)
    return layer, torch.randn(*shape, cin, generator=g).to(gpu), torch.randn(*shape, c, generator=g).to(gpu)


LAYER_CLASSES = {"image": layers.Batch_Image_ZERON_GCNGCN, "batch": layers.BatchZERON_GCN, "unbatched": layers.ZERON_GCN}


def _layer_cases():
    from test_products_gpu import SHAPES
    seen = set()
    for cname in LAYER_CLASSES:
        for b, cin, c in SHAPES:
            key = (cname, 1 if cname == "unbatched" else b, cin, c)
            if key not in seen:
                seen.add(key)
                yield key


@pytest.mark.parametrize("aname", list(ACTIVATIONS))
@pytest.mark.parametrize("own", [False, True], ids=["library", "own"])
@pytest.mark.parametrize("cname,b,cin,c", list(_layer_cases()), ids=["%s-%dx%d->%d" % (n, 162 * b, cin, c) for n, b, cin, c in _layer_cases()])
def test_layers_carry_planted_values_on_every_product_route(gpu, meshes, monkeypatch, cname, b, cin, c, own, aname):
    """Batch_Image_ZERON_GCNGCN, BatchZERON_GCN and ZERON_GCN at the shapes of tests/test_products_gpu.py (one per route of
    products.route()), the library's products and the package's own preferred: forward, grad_x, grad_weight and grad_bias
    against ref_ops.zero_n_layer(aggregate=sparse) under float64 autograd.  Values planted in the layer's INPUT, in its first
    and its last column (the last k-step of a product whose depth is no multiple of the tile's).  An upstream gradient element
    whose pre-activation sits on the ReLU's kink is zero on both sides."""
    from geometrics_amd import products
    from test_products_gpu import ROUTES, issued
    _, csr, a64, where = meshes["ico162"]
    cls, (activation, act, activation64) = LAYER_CLASSES[cname], ACTIVATIONS[aname]
    layer, x0, seed0 = _layer_case(gpu, cls, b, cin, c, 3 * cin + c)
    w64, b64 = layer._weight().detach().double().cpu().reshape(cin, c), layer.bias.detach().double().cpu()
    batched = x0.dim() == 3
    lead = (lambda t: t if batched else t.unsqueeze(0))
    mesh = (x0.shape[0] if batched else 1, csr, a64, where)
    # the kink: |pre| within twice the forward bound of zero, on the un-planted input (a planted value moves no finite element)
    pre64 = ref_ops.zero_n_layer(x0.double().cpu(), a64, w64, b64, layer.split, lambda t: t, aggregate=ref_ops.sparse_aggregate)
    m0 = _layer_masses(a64, x0.double().cpu(), w64, b64, layer.split, pre64, seed0, 0)
    if act == 1:
        knife = pre64.abs() <= 2 * LAYER_RTOL * m0["out"]
        assert float(knife.double().mean()) <= BN_MAX_KNIFE
        seed0 = seed0 * (~knife).to(gpu)
    monkeypatch.setattr(products, "own_dense_products", own)
    recorded = False
    for label, cells in plants(mesh, (("first", 0), ("last", cin - 1))):
        x = planted(lead(x0), cells).reshape(x0.shape).requires_grad_(True)

        def step():
            x.grad = None
            for p in layer.parameters():
                p.grad = None
            step.out = layer(x, csr, activation)
            step.out.backward(seed0)
            torch.cuda.synchronize()
        if not recorded and cname == "image":        # the route this shape is in the table for did run, non-finite input and all
            events = issued(step, monkeypatch)
            key = ("%dx%d->%d" % (162 * b, cin, c), "plain", own)
            assert events == [line.strip().replace("(b) ", "") for line in ROUTES[key].strip().split("\n")], (label, events)
            recorded = True
        else:
            step()
        x64 = x.detach().double().cpu().requires_grad_(True)
        w, bias = w64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
        out64 = ref_ops.zero_n_layer(x64, a64, w, bias, layer.split, activation64, aggregate=ref_ops.sparse_aggregate)
        out64.backward(seed0.double().cpu())
        mass = _layer_masses(a64, x64.detach(), w64, b64, layer.split, out64.detach(), seed0, act)
        got = {"out": step.out, "grad_x": x.grad, "grad_weight": layer._weight().grad.reshape(cin, c), "grad_bias": layer.bias.grad}
        want = {"out": out64.detach(), "grad_x": x64.grad, "grad_weight": w.grad, "grad_bias": bias.grad}
        assert not bool(torch.isfinite(want["grad_weight"]).all()) and bool(torch.isfinite(want["grad_x"]).any())
        for name in got:
            nonfinite_close(got[name], want[name], mass[name], BIAS_RTOL if name == "grad_bias" else LAYER_RTOL,
                            "%s %s %s, %s: %s" % (cname, aname, "own" if own else "library", label, name))


@pytest.mark.parametrize("aname", list(ACTIVATIONS))
@pytest.mark.parametrize("own", [False, True], ids=["library", "own"])
def test_a_stack_across_two_fused_boundaries_carries_planted_values(gpu, meshes, monkeypatch, own, aname):
    """tests/test_products_gpu.py's `stack` mode: three 192-wide layers whose two boundaries are single launches
    (geom_zn_layer_{fwd,bwd}_f32), against three ref_ops.zero_n_layer(aggregate=sparse) under float64 autograd.  The forward
    element by element (three layers' bounds, each layer's mass carried into the next); behind three ReLUs a hidden unit on the
    kink may switch, so the gradients' finite elements are held in the max-norm at the 2e-3 of
    tests/test_aggregate_route_gpu.py's stack -- under ELU, which has no kink, at 5e-5 of scale --, their non-finite elements kind by
    kind."""
    from geometrics_amd import fused, products
    from test_products_gpu import ROUTES, issued
    batch, (_, csr, a64, where) = 4, meshes["ico162"]
    activation, act, activation64 = ACTIVATIONS[aname]
    torch.manual_seed(17)
    stack = [layers.Batch_Image_ZERON_GCNGCN(192, 192).to(gpu) for _ in range(3)]
    g = torch.Generator(device="cpu").manual_seed(18)
    x0, seed = torch.randn(batch, 162, 192, generator=g).to(gpu), torch.randn(batch, 162, 192, generator=g).to(gpu)
    params64 = [(l.weight1.detach().double().cpu()[0], l.bias.detach().double().cpu()) for l in stack]
    monkeypatch.setattr(products, "own_dense_products", own)
    monkeypatch.setattr(fused, "force", {"fwd": True, "bwd": True})
    recorded = False
    for label, cells in plants((batch, csr, a64, where), (("first", 0), ("last", 191))):
        x = planted(x0, cells).requires_grad_(True)
        leaves = [x] + [p for l in stack for p in l.parameters()]

        def step():
            for p in leaves:
                p.grad = None
            step.out = layers.zero_n_stack(x, csr, stack, activation)
            step.out.backward(seed)
            torch.cuda.synchronize()
        if not recorded and aname == "relu":
            events = issued(step, monkeypatch)
            assert events == [line.strip() for line in ROUTES[("3x(648x192->192)", "stack", own)].strip().split("\n")], events
            recorded = True
        else:
            step()
        x64 = x.detach().double().cpu().requires_grad_(True)
        leaves64 = [(w.clone().requires_grad_(True), bias.clone().requires_grad_(True)) for w, bias in params64]
        h, mass = x64, finite_part(x64.detach()).abs()
        for w, bias in leaves64:
            h = ref_ops.zero_n_layer(h, a64, w, bias, 3, activation64, aggregate=ref_ops.sparse_aggregate)
            mass = _aggregate64(a64.abs(), mass @ w.detach().abs(), 64) + bias.detach().abs()
            mass = torch.maximum(mass, finite_part(h.detach()).abs())          # (elu(-Inf) = -1 stays in the mass)
        h.backward(seed.double().cpu())
        nonfinite_close(step.out, h.detach(), mass, 3 * LAYER_RTOL, "stack %s, %s: out" % (aname, label))
        got = [x.grad] + [p.grad for l in stack for p in (l.weight1, l.bias)]
        want = [x64.grad] + [t.grad for pair in leaves64 for t in pair]
        assert not all(bool(torch.isfinite(t).all()) for t in want)
        for i, (a, e) in enumerate(zip(got, want)):
            scale = finite_part(e).abs().max() * torch.ones_like(e)
            nonfinite_close(a.reshape(e.shape), e, scale, 2e-3 if act == 1 else 5e-5, "stack %s, %s: gradient %d" % (aname, label, i))


# ---- d. BatchMeshDeformationBlock -----------------------------------------------------------------------------------------------------
BLOCK_FWD_RTOL = 2e-5       # of the tensor's scale: the forward bar of tests/test_deform_gpu.py


def _hops_from(a64, v):
    """Ring distance of every vertex from v over the adjacency's pattern (-1: not reached)."""
    pattern = (a64 != 0) | (a64.t() != 0)
    dist = torch.full((a64.shape[0],), -1, dtype=torch.long)
    front, d = torch.zeros(a64.shape[0], dtype=torch.bool), 0
    front[v] = True
    while bool(front.any()):
        dist[front] = d
        front, d = pattern[front].any(0) & (dist < 0), d + 1
    return dist


def _block_case(case, gpu, batch=None):
    """(block on the device, features, pooled, dense adjacency, its float64 copy) of a case of tests/golden/block192.npz; batch:
    another batch size, its inputs drawn by the fixture's scheme."""
    from geometrics_amd import models
    from helpers import block192_case, block192_fixture, block192_parameters, seeded_input
    g = block192_fixture(case)
    nv, seed = int(g["nv"]), int(g["seed"])
    inp = block192_case(g) if batch is None else {"features": seeded_input([seed, 0], (batch, nv, 3)),
                                                  "pooled": seeded_input([seed, 3], (batch, nv, 192))}
    faces = meshgen.uv_sphere()[1] if str(g["mesh"]) == "uv_sphere_482" else meshgen.icosphere(2)[1]
    adj = utils.adj_init(torch.from_numpy(faces).to(gpu))["adj"]
    block = block192_parameters(models.BatchMeshDeformationBlock(195, nv), g).to(gpu)
    return block, torch.from_numpy(inp["features"]).to(gpu), torch.from_numpy(inp["pooled"]).to(gpu), adj, adj.double().cpu()


def _block_plants(a64, batch, far):
    """One NaN, then one +Inf, in `features`, then in `pooled`.  far: at the vertex farthest from any other (482 vertices: 14
    layers do not reach its antipode), else at an ordinary one."""
    v = int(torch.stack([_hops_from(a64, u).max() for u in range(0, a64.shape[0], 7)]).argmax()) * 7 if far else a64.shape[0] // 3
    for operand, col in (("features", 1), ("pooled", 100)):
        for name, value in (("nan", NAN), ("+inf", INF)):
            yield "%s in %s at vertex %d" % (name, operand, v), operand, [(batch // 2, v, col, value)], v


def _mask_close(got, want, what):
    """The non-finite mask at every element (kinds=False), the finite elements at the forward bar of the finite tests."""
    for name, a, e in zip(("features", "coords"), got, want):
        scale = finite_part(e).abs().max() * torch.ones_like(e)
        nonfinite_close(a, e, scale, BLOCK_FWD_RTOL, "%s: %s" % (what, name), kinds=False)


def _spy(monkeypatch, module, names):
    calls = []
    for name in names:
        real = getattr(module, name)

        def spy(*a, _real=real, _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(module, name, spy)
    return calls


@pytest.mark.parametrize("case", ["ico162_bn", "train482"])
def test_the_deformation_block_carries_planted_values_on_every_training_route_and_in_eval(gpu, monkeypatch, case):
    """The fused launches per layer, the chain launches, the separate operators (deform.enabled = False) and the eval-mode
    launches under no_grad against helpers.block64(aggregate=sparse).  Training: one statistic per vertex, so a non-finite
    value takes the vertex's row of EVERY mesh and spreads one ring per layer; eval: it stays in its mesh.  On the 482-vertex
    mesh it is planted where 14 layers do not reach every vertex: the exact reach is compared, not `everything is NaN`."""
    import copy
    from geometrics_amd import deform
    from helpers import block64
    block, feats0, pooled0, adj, a64 = _block_case(case, gpu)
    csr = layers.adjacency_csr(adj)
    far = case == "train482"
    calls = _spy(monkeypatch, deform, ("chain_forward", "layer_forward", "infer_layer_forward"))
    running = {i: (getattr(block, "bn%d" % i).running_mean.double().cpu(), getattr(block, "bn%d" % i).running_var.double().cpu())
               for i in range(1, 14)}
    for label, operand, cells, v in _block_plants(a64, feats0.shape[0], far):
        feats = planted(feats0, cells) if operand == "features" else feats0
        pooled = planted(pooled0, cells) if operand == "pooled" else pooled0
        with torch.no_grad():
            want = block64(block, feats.double().cpu(), pooled.double().cpu(), a64, aggregate=ref_ops.sparse_aggregate)[:2]
            want_eval = block64(block, feats.double().cpu(), pooled.double().cpu(), a64, running=running,
                                aggregate=ref_ops.sparse_aggregate)[:2]
        bad_rows = ~torch.isfinite(want[1]).all(-1)
        assert bool(bad_rows.any()) and bool((bad_rows == bad_rows[0]).all())          # the same vertices of every mesh
        if far:
            hops = _hops_from(a64, v)
            assert int(hops.max()) >= 15
            assert bool(torch.equal(~torch.isfinite(want[0]).all(-1)[0], hops <= 13)) and bool(torch.equal(bad_rows[0], hops <= 14))
            assert bool((~bad_rows).any())
        b = cells[0][0]
        others = torch.arange(feats0.shape[0]) != b
        assert not bool(torch.isfinite(want_eval[1][b]).all()) and bool(torch.isfinite(want_eval[1][others]).all())
        for route in ("per layer", "chain", "separate"):
            blk = copy.deepcopy(block).train()
            monkeypatch.setattr(deform, "enabled", route != "separate")
            monkeypatch.setattr(deform, "chain", route == "chain")
            assert deform.serves(blk, feats, pooled, csr) == (route != "separate")
            del calls[:]
            got = blk(feats.clone().requires_grad_(True), pooled.clone().requires_grad_(True), adj)
            torch.cuda.synchronize()
            assert calls == {"per layer": ["layer_forward"] * 13, "chain": ["chain_forward"], "separate": []}[route]
            _mask_close(got, want, "%s, %s" % (route, label))
        for route in ("fused", "separate"):
            blk = copy.deepcopy(block).eval()
            monkeypatch.setattr(deform, "enabled", route == "fused")
            del calls[:]
            with torch.no_grad():
                assert deform.serves_inference(blk, feats, pooled, csr) == (route == "fused")
                got = blk(feats, pooled, adj)
            torch.cuda.synchronize()
            assert calls == (["infer_layer_forward"] * 13 if route == "fused" else [])
            _mask_close(got, want_eval, "eval %s, %s" % (route, label))


def test_the_wide_deformation_route_carries_planted_values(gpu, monkeypatch):
    """Batch 17 on the 482-vertex mesh: the launches with two row tiles per vertex (deform.wide) and the separate operators."""
    import copy
    from geometrics_amd import deform
    from helpers import block64
    block, feats0, pooled0, adj, a64 = _block_case("train482", gpu, batch=17)
    csr = layers.adjacency_csr(adj)
    calls = _spy(monkeypatch, deform, ("wide_layer_forward", "layer_forward", "chain_forward"))
    for label, operand, cells, v in _block_plants(a64, 17, True):
        feats = planted(feats0, cells) if operand == "features" else feats0
        pooled = planted(pooled0, cells) if operand == "pooled" else pooled0
        with torch.no_grad():
            want = block64(block, feats.double().cpu(), pooled.double().cpu(), a64, aggregate=ref_ops.sparse_aggregate)[:2]
        bad_rows = ~torch.isfinite(want[1]).all(-1)
        assert bool(bad_rows.any()) and bool((~bad_rows).any())
        for wide in (True, False):
            blk = copy.deepcopy(block).train()
            monkeypatch.setattr(deform, "wide", wide)
            monkeypatch.setattr(deform, "enabled", wide)
            assert deform.serves_wide(blk, feats, pooled, csr) == wide and not deform.serves(blk, feats, pooled, csr)
            del calls[:]
            got = blk(feats.clone().requires_grad_(True), pooled.clone().requires_grad_(True), adj)
            torch.cuda.synchronize()
            assert calls == (["wide_layer_forward"] * 13 if wide else [])
            _mask_close(got, want, "%s, %s" % ("wide" if wide else "separate", label))


# ---- e. MeshDeformationBlock (unbatched, no BatchNorm) ------------------------------------------------------------------------------------
def _plain_block64(params, feats, pooled, a64):
    """models.MeshDeformationBlock.forward (reference models.py:138-201) in float64 on the rows' stored entries."""
    from geometrics_amd import deform
    layer = lambda i, x, act: ref_ops.zero_n_layer(x, a64, params["gc%d.weight1" % i], params["gc%d.bias" % i], 3, act,
                                                   aggregate=ref_ops.sparse_aggregate)
    full = torch.cat((feats, pooled), dim=1)
    x, outs = full, {"lead": full[:, :192]}
    for i, src, _, _, tap in deform.SCHEDULE:
        x = layer(i, x, F.relu)
        if src is not None:
            x = (outs.pop(src) + x) / 2
        if tap:
            outs[i] = x
    return x, layer(15, x, lambda t: t)


@pytest.mark.parametrize("which", ["b", "d"], ids=["uv_sphere_482", "split_519_row_of_65"])
def test_the_plain_deformation_block_carries_planted_values(gpu, monkeypatch, which):
    """geom_deform_plain_{fwd,bwd}_f32 through models.MeshDeformationBlock on the 482-vertex sphere (33-entry poles) and on the
    split mesh with a row of 65 entries (tests/deform_plain_helpers.launch_adjacency), against the float64 block on the rows'
    stored entries.  There is no normalisation, so NaN, +Inf and -Inf are compared kind by kind, in the outputs and in every
    gradient.  The finite elements: the forward at the finite tests' 2e-5 of scale; the gradients, thirteen ReLUs deep, in the
    L2 norm at the 5e-3 tests/test_deform_gpu.py holds a block under ReLU to (a unit on the kink may switch)."""
    import deform_plain_helpers as dph
    from geometrics_amd import deform, models
    monkeypatch.setattr(deform, "plain", True)
    adj = torch.from_numpy(dph.launch_adjacency(which)).to(gpu)
    a64, nv = adj.double().cpu(), adj.shape[0]
    lens = (a64 != 0).sum(1)
    assert int(lens.max()) == (33 if which == "b" else 65)
    block = dph.fill_plain_parameters(models.MeshDeformationBlock(195), 4200 + ord(which)).to(gpu)
    inputs = dph.case_inputs(4300 + ord(which), nv)
    to = lambda k: torch.from_numpy(inputs[k]).to(gpu)
    feats0, pooled0, g_f, g_c = to("features"), to("pooled"), to("g_features"), to("g_coords")
    assert deform.serves_plain(block, feats0, pooled0, layers.adjacency_csr(adj))
    params = {k: v.detach().double().cpu() for k, v in block.named_parameters()}
    mesh = (1, None, a64, [("ordinary", nv // 3), ("longest row", int(lens.argmax())), ("last", nv - 1)])
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for label, cells in plants(mesh, (("lead", 0), ("beyond the lead", 191))):          # columns 3 and 194 of the block's input
        pooled = planted(pooled0.unsqueeze(0), cells)[0].requires_grad_(True)
        feats = feats0.clone().requires_grad_(True)
        for p in block.parameters():
            p.grad = None
        del calls[:]
        out_f, coords = block(feats, pooled, adj)
        ((out_f * g_f).sum() + (coords * g_c).sum()).backward()
        torch.cuda.synchronize()
        assert calls.count("geom_deform_plain_fwd_f32") == 13 and calls.count("geom_deform_plain_bwd_f32") == 13
        f64, p64 = feats.detach().double().cpu().requires_grad_(True), pooled.detach().double().cpu().requires_grad_(True)
        leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        e_f, e_c = _plain_block64(leaves, f64, p64, a64)
        ((e_f * g_f.double().cpu()).sum() + (e_c * g_c.double().cpu()).sum()).backward()
        assert not bool(torch.isfinite(e_c).all())
        for name, got, want in (("features", out_f, e_f.detach()), ("coords", coords, e_c.detach())):
            scale = finite_part(want).abs().max() * torch.ones_like(want)
            nonfinite_close(got, want, scale, dph.FORWARD_BAR, "plain block %s, %s: %s" % (which, label, name))
        grads = [("grad.features", feats.grad, f64.grad), ("grad.pooled", pooled.grad, p64.grad)]
        grads += [("grad." + k, p.grad, leaves[k].grad) for k, p in block.named_parameters()]
        for name, got, want in grads:
            what = "plain block %s, %s: %s" % (which, label, name)
            nonfinite_close(got, want, torch.full_like(want, 1e300), 1.0, what)                    # (the mask and the kinds)
            fin = torch.isfinite(want)
            if bool(fin.any()):
                err = float((got.double().cpu()[fin] - want[fin]).norm()) / max(float(want[fin].norm()), 1e-300)
                assert err <= 5e-3, "%s: the finite elements are %.2e from float64 in the L2 norm" % (what, err)


# ---- f. the frozen BatchMeshEncoder on the fused route ---------------------------------------------------------------------------------------
def test_the_frozen_encoder_keeps_a_nan_position_through_the_vertex_max(gpu):
    """ico162_b2 of tests/golden/batch_mesh_encoder.npz with a NaN in one position: sixteen ELU layers and the head on one
    launch per layer, then the max over the vertices, which keeps the NaN as torch.max does.  The mask of pre_max and of the
    latents against the float64 restatement on the rows' stored entries; the other mesh at the finite test's 2e-5 of scale."""
    import test_batch_encoder_gpu as tbe
    from geometrics_amd import encoder
    c = tbe._case(golden("batch_mesh_encoder"), "ico162_b2")
    enc = tbe._encoder(c)
    pos, adj = tbe._inputs(c)
    pos = planted(pos, [(1, pos.shape[1] // 3, 1, NAN)])
    was, encoder.enabled = encoder.enabled, True
    try:
        with torch.no_grad():
            v = enc.pre_max(pos, adj)
            assert enc.last_route == "fused"
            lat = enc(pos, adj)
            assert enc.last_route == "fused"
    finally:
        encoder.enabled = was
    params = {k: p.detach().double().cpu() for k, p in enc.named_parameters()}
    a64, x = adj.double().cpu(), pos.double().cpu()
    for name in ref_ops.ENCODER_LAYERS:
        x = ref_ops.zero_n_layer(x, a64, params[name + ".weight"], params[name + ".bias"], 10, F.elu, aggregate=ref_ops.sparse_aggregate)
    v64 = ref_ops.zero_n_layer(x, a64, params["reduce.weight_Ws.0"], params["reduce.weight_Bs.0"], 10, lambda t: t,
                               aggregate=ref_ops.sparse_aggregate)
    lat64 = v64.max(dim=1)[0]
    assert bool(torch.isnan(lat64[1]).all()) and bool(torch.isfinite(lat64[0]).all()) and bool(torch.isfinite(v64[0]).all())
    for name, got, want in (("pre_max", v, v64), ("latents", lat, lat64)):
        scale = finite_part(want).abs().max() * torch.ones_like(want)
        nonfinite_close(got, want, scale, tbe.VALUE_BAR, "encoder " + name, kinds=False)


# ---- g. the losses ----------------------------------------------------------------------------------------------------------------------------
def _nan_exactly_when(loss, ref, what):
    got, want = float(loss), float(ref)
    assert np.isnan(got) == np.isnan(want), "%s: the loss is %r, the float64 / oracle restatement %r" % (what, got, want)
    if not np.isnan(want):
        assert abs(got - want) <= 1e-5 * abs(want), (what, got, want)
    return np.isnan(want)


def test_a_nan_vertex_ends_as_nan_in_the_surface_losses(gpu):
    """One NaN coordinate in one predicted vertex of tests/golden/p2s_v162.npz.  batch_point_to_surface and batch_point_to_point
    on the fixture's draws, then batch_point_to_surface on the draws the package generates itself -- plain, with gt_index=, and
    with the finalize pass inside the scan launch or in a launch of its own --, each replayed through ref_ops on the SAME draws:
    the loss is NaN exactly when the restatement's is (a sample drawn on a face of the vertex), and a finite one agrees."""
    from geometrics_amd import ops
    g = golden("p2s_v162")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    verts = planted(to(g["verts"]), [(0, 40, 1, NAN)])
    faces, gt = to(g["faces"]), to(g["gt"])
    info = {"faces": faces}
    cpu = lambda t: t.detach().cpu()
    fixture = tuple(to(g[k]) for k in ("choices", "u", "v"))
    seen = []
    for fn, ref_fn in (("batch_point_to_surface", ref_ops.point_to_surface), ("batch_point_to_point", ref_ops.point_to_point)):
        with torch.no_grad():
            loss = getattr(utils, fn)(verts, info, gt, num=fixture[0].shape[1], draws=fixture)
        ref = ref_fn(cpu(verts), cpu(faces).long(), cpu(gt), *(cpu(t) for t in fixture))
        seen.append(_nan_exactly_when(loss, ref, fn + " on the fixture's draws"))
    assert all(seen)                                      # the fixture's 500 samples do touch the vertex's faces
    num, n_gt = 500, gt.shape[1]
    tail_was = ops.scan_finalize_tail
    try:
        for index, tail in ((False, True), (True, True), (True, False)):
            ops.scan_finalize_tail = tail
            ops.manual_seed(5)
            gi = ops.GtIndex(gt) if index else None
            with torch.no_grad():
                d = ops.draw_samples(verts, faces, num, with_points=True, prepare_scan_for=n_gt, gt_index=gi)
                loss = ops.SurfaceLoss.apply(verts, faces, gt, d[0], d[1], d[2], False, 3000.0, d[3], d[4], None, gi)[0]
            torch.cuda.synchronize()
            ref = ref_ops.point_to_surface(cpu(verts), cpu(faces).long(), cpu(gt), cpu(d[0]).long(), cpu(d[1]), cpu(d[2]))
            _nan_exactly_when(loss, ref, "batch_point_to_surface on its own draws (gt_index %s, finalize tail %s)" % (index, tail))
            assert not ops.finalize_roles_gave_up()
    finally:
        ops.scan_finalize_tail = tail_was
        ops.manual_seed(0, gpu)


def test_a_nan_vertex_ends_as_nan_in_the_stage_regularisers(gpu):
    from helpers import stage_regularisers_chain
    from test_ops_parity_gpu import STAGE_REG_CASES, stage_regulariser_case
    prev, cur, faces, adj_orig, weights = stage_regulariser_case(STAGE_REG_CASES[2])
    b, nv, nf = cur.shape[0], cur.shape[1], faces.shape[0]
    coef = (weights[0] / (b * nv), weights[1] / (b * nv), weights[2] / (3.0 * b * nf))
    info = {"adj_orig": adj_orig.to(gpu), "faces": faces.to(gpu)}
    for planted_cur in (False, True):
        c = planted(cur, [(0, nv // 2, 2, NAN)]) if planted_cur else cur
        with torch.no_grad():
            loss = utils.stage_regularisers(prev.to(gpu), c.to(gpu), info, *weights)
        ref = stage_regularisers_chain(prev.double(), c.double(), adj_orig.double(), faces, *coef, 1.0)["value"]
        assert _nan_exactly_when(loss, ref, "stage_regularisers") == planted_cur
