"""-m gpu: training batches of 17 .. 64 meshes on the fused deformation block (geom_deform_layer_wide_{fwd,bwd}_f32,
deform.serves_wide): one workgroup per vertex, its b rows as ceil(b / 16) row tiles behind one register-resident weight slice.

The batches are the smallest at which the tiling can go wrong: 17 (one live row in tile 2), 33 (one live row in tile 3), 64 (four
full tiles) on the pole-free icosphere, and 24 on the 482-vertex template (its two 33-entry poles go through the tail table with
a half-full second tile).

* one forward / one backward launch against the separate operators (aggregation bits identical) and float64;
* the whole block against float64 (helpers.block64) and against the separate operators, with the launches counted;
* case ico162_b24 of tests/golden/block192.npz (the reference's own block in float64) on the wide route;
* two eager steps and a HIP-graph replay give the same bits; routing.

The bars are the ones the project holds at b <= 16 (test_deform_gpu.py): 2e-6 for x and the residual's gradient, 1e-5 for the
statistics, 1e-4 for the BatchNorm backward's outputs, 2e-5 / 5e-5 / 5e-3 (L2) for the block.  Every margin goes through
helpers.log_margin (GEOM_MARGIN_LOG).  The products and the head are held to the fp32 summation bound of their term count:
(terms + 8) * 2^-24 * sum |a| |b| per element."""
import copy

import numpy as np
import pytest
import torch

from geometrics_amd import _lib, deform, layers, meshgen, models, utils
from helpers import bits, block192_case, block192_fixture, block192_parameters, block192_stored, log_margin, weighted_checksum
from helpers import bn64 as _bn64, block64 as _block64

pytestmark = pytest.mark.gpu

@pytest.fixture(autouse=True)
def _wide_on(monkeypatch):
    """The tests hold the wide route itself, whatever the switch's default is."""
    monkeypatch.setattr(deform, "wide", True)


SHAPES = [("icosphere_162", 17), ("icosphere_162", 33), ("icosphere_162", 64), ("uv_sphere_482", 24)]
_MESHES = {}


def _mesh(name, gpu):
    if name not in _MESHES:
        V, Fc = meshgen.uv_sphere() if name == "uv_sphere_482" else meshgen.icosphere(2)
        adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
        _MESHES[name] = (V.shape[0], adj, layers.adjacency_csr(adj))
    return _MESHES[name]


def _maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _l2rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def _within(what, got, want, bound):
    """|got - want| <= bound element by element; logged as the worst element's share of its bound."""
    worst = float(((got.double().cpu() - want).abs() / (bound + 1e-30)).max())
    return log_margin(what, worst, 1.0)


def _d(t):
    return t.detach().double().cpu()


@pytest.mark.parametrize("mesh,batch", SHAPES)
def test_one_wide_forward_launch_against_the_separate_operators(gpu, mesh, batch):
    nv, adj, csr = _mesh(mesh, gpu)
    tag = "wide fwd %s b%d " % (mesh, batch)
    torch.manual_seed(3)
    c = 192
    s = torch.randn(batch, nv, c, device=gpu)
    bias = torch.randn(c, device=gpu) * 0.1
    gamma, beta = torch.rand(nv, device=gpu) + 0.5, torch.randn(nv, device=gpu) * 0.2
    wide_res = torch.randn(batch, nv, c + 11, device=gpu)
    res = wide_res[..., 4:4 + c]              # a column slice of a wider buffer: read in place at its pitch (4-byte aligned)
    w = torch.randn(c, c, device=gpu) / 14
    rm, rv = torch.zeros(nv, device=gpu), torch.ones(nv, device=gpu)
    z, x, s_next = (torch.full_like(s, float("nan")) for _ in range(3))
    mean, invstd = torch.empty(nv, device=gpu), torch.empty(nv, device=gpu)
    packed, _ = deform.pack_weights([w])
    res_op, res_ld = deform.rows_operand(res, (batch, nv, c))
    assert res_op.data_ptr() == res.data_ptr() and res_ld == c + 11
    deform.wide_layer_forward(s, bias, csr, gamma, beta, rm, rv, True, 0.1, 1e-5, True, res, 0.5, z, x, mean, invstd,
                              w_next=packed[0], s_out=s_next)
    # aggregation: the bits of the stand-alone operator
    assert torch.equal(z, layers.zero_n_aggregate(s, adj, bias, 64, None))
    # BatchNorm + ReLU + residual average, and the product, against float64
    y64, m64, v64 = _bn64(_d(z), _d(gamma), _d(beta), 1e-5)
    x64 = (_d(res) + torch.relu(y64)) * 0.5
    assert log_margin(tag + "x", _maxrel(x, x64), 2e-6)
    assert log_margin(tag + "save_mean", _maxrel(mean, m64), 1e-5)
    assert log_margin(tag + "save_invstd", _maxrel(invstd, 1.0 / torch.sqrt(v64 + 1e-5)), 1e-5)
    n = batch * c
    assert log_margin(tag + "running_mean", _maxrel(rm, 0.1 * m64), 1e-5)
    assert log_margin(tag + "running_var", _maxrel(rv, 0.9 + 0.1 * v64 * n / (n - 1)), 1e-5)
    assert _within(tag + "product", s_next, _d(x) @ _d(w), (c + 8) * 2.0 ** -24 * (_d(x).abs() @ _d(w).abs()))
    # no product: the last hidden layer, with the coordinate head's product in the launch
    x2 = torch.full_like(s, float("nan"))
    w_head = torch.randn(c, 3, device=gpu) / 14
    s_head = torch.full((batch, nv, 3), float("nan"), device=gpu)
    rm2, rv2 = rm.clone(), rv.clone()
    deform.wide_layer_forward(s, bias, csr, gamma, beta, rm2, rv2, True, 0.1, 1e-5, True, None, 0.5, None, x2, mean, invstd,
                              w_head=w_head, s_head=s_head)
    assert log_margin(tag + "x (no product)", _maxrel(x2, torch.relu(y64)), 2e-6)
    assert _within(tag + "head", s_head, _d(x2) @ _d(w_head), (c + 8) * 2.0 ** -24 * (_d(x2).abs() @ _d(w_head).abs()))
    assert log_margin(tag + "running_mean (second step)", _maxrel(rm2, 0.19 * m64), 1e-5)
    # training = False: the launch normalises with the running statistics and writes nothing to them
    rm3, rv3 = torch.randn(nv, device=gpu) * 0.3, torch.rand(nv, device=gpu) + 0.5
    keep = (rm3.clone(), rv3.clone())
    x3 = torch.full_like(s, float("nan"))
    deform.wide_layer_forward(s, bias, csr, gamma, beta, rm3, rv3, False, 0.1, 1e-5, True, res, 0.5, None, x3, None, None,
                              w_next=packed[0], s_out=s_next)
    y3 = (_d(z) - _d(rm3).view(1, -1, 1)) / torch.sqrt(_d(rv3).view(1, -1, 1) + 1e-5) * _d(gamma).view(1, -1, 1) + _d(beta).view(1, -1, 1)
    assert log_margin(tag + "x (running statistics)", _maxrel(x3, (_d(res) + torch.relu(y3)) * 0.5), 2e-6)
    assert torch.equal(rm3, keep[0]) and torch.equal(rv3, keep[1])
    assert _within(tag + "product (running statistics)", s_next, _d(x3) @ _d(w), (c + 8) * 2.0 ** -24 * (_d(x3).abs() @ _d(w).abs()))


@pytest.mark.parametrize("mesh,batch", SHAPES)
def test_one_wide_backward_launch_against_the_separate_operators(gpu, mesh, batch):
    nv, adj, csr = _mesh(mesh, gpu)
    tag = "wide bwd %s b%d " % (mesh, batch)
    torch.manual_seed(4)
    c = 192
    shape = (batch, nv, c)
    dz_up, z = (torch.randn(*shape, device=gpu) for _ in range(2))
    g2 = torch.randn(batch, nv, c + 7, device=gpu)[..., 3:3 + c]      # read in place at its pitch
    wt = torch.randn(c, c, device=gpu) / 14
    gamma, beta = torch.rand(nv, device=gpu) + 0.5, torch.randn(nv, device=gpu) * 0.2
    z64 = _d(z)
    mean64 = z64.mean(dim=(0, 2))
    var64 = ((z64 - mean64.view(1, -1, 1)) ** 2).mean(dim=(0, 2))
    mean, invstd = mean64.float().to(gpu), (1.0 / torch.sqrt(var64 + 1e-5)).float().to(gpu)
    ds, dz, gres = (torch.full(shape, float("nan"), device=gpu) for _ in range(3))
    gbw, gbb = torch.empty(nv, device=gpu), torch.empty(nv, device=gpu)
    colsum = torch.empty(nv, c, device=gpu)
    _, packed_t = deform.pack_weights([wt.t().contiguous()])      # the launch reads the layer's weight transposed, packed
    deform.wide_layer_backward(shape, csr, z, gamma, beta, mean, invstd, True, True, 0.5, dz, gbw, gbb, dz_up=dz_up, ds_up=ds,
                               wt_up=packed_t[0], g2=g2, grad_res=gres, colsum=colsum)
    ds_ref, _ = layers.aggregate_backward(dz_up, csr, 64, layers._ACT_NONE, None, None, False)
    assert torch.equal(ds, ds_ref)
    # float64 from here: dX = dS . W^T (wt IS the transposed weight), + g2, residual scale, ReLU mask, BatchNorm backward
    gx = (_d(ds) @ _d(wt) + _d(g2)) * 0.5
    assert log_margin(tag + "grad_res", _maxrel(gres, gx), 2e-6)
    m, i = _d(mean).view(1, -1, 1), _d(invstd).view(1, -1, 1)
    xh = (z64 - m) * i
    ga, be = _d(gamma).view(1, -1, 1), _d(beta).view(1, -1, 1)
    # (the mask is formed in fp32, operation by operation as the kernel forms it -- and as the forward launch formed its ReLU)
    on = ((((z - mean.view(1, -1, 1)) * invstd.view(1, -1, 1)) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)) > 0).cpu()
    n = batch * c

    def bn_backward(gy):
        sg, sgx = gy.sum(dim=(0, 2)), (gy * xh).sum(dim=(0, 2))
        return sg, sgx, ga * i * (gy - sg.view(1, -1, 1) / n - xh * sgx.view(1, -1, 1) / n)
    sg, sgx, dz64 = bn_backward(torch.where(on, gx, torch.zeros_like(gx)))
    assert log_margin(tag + "grad_bn_b", _maxrel(gbb, sg), 1e-4) and log_margin(tag + "grad_bn_w", _maxrel(gbw, sgx), 1e-4)
    assert log_margin(tag + "dz", _maxrel(dz, dz64), 1e-4)
    assert log_margin(tag + "colsum", _maxrel(colsum, dz64.sum(dim=0)), 1e-4)
    # no product: the gradient of the output is read from memory (+ the second one)
    g = torch.randn(*shape, device=gpu)
    dz2 = torch.full(shape, float("nan"), device=gpu)
    deform.wide_layer_backward(shape, csr, z, gamma, beta, mean, invstd, True, False, 0.5, dz2, gbw, gbb, g=g, g2=g2)
    _, _, want = bn_backward(torch.where(on, _d(g) + _d(g2), torch.zeros_like(gx)))
    assert log_margin(tag + "dz (no product)", _maxrel(dz2, want), 1e-4)
    # the top layer with the coordinate head: g += ds_head . w_head^T, dw_head[v] = x_top[:, v]^T . ds_head[:, v]
    ds_head = torch.randn(batch, nv, 3, device=gpu)
    w_head = torch.randn(c, 3, device=gpu) / 14
    x_top = torch.randn(*shape, device=gpu)
    dw_head = torch.full((nv, c * 3), float("nan"), device=gpu)
    dz3 = torch.full(shape, float("nan"), device=gpu)
    gres3 = torch.full(shape, float("nan"), device=gpu)
    deform.wide_layer_backward(shape, csr, z, gamma, beta, mean, invstd, True, True, 0.5, dz3, gbw, gbb, g=g, grad_res=gres3,
                               colsum=colsum, ds_head=ds_head, w_head=w_head, x_top=x_top, dw_head=dw_head)
    g_top = (_d(g) + _d(ds_head) @ _d(w_head).t()) * 0.5
    assert log_margin(tag + "grad_res (head)", _maxrel(gres3, g_top), 2e-6)
    sg, sgx, want = bn_backward(torch.where(on, g_top, torch.zeros_like(gx)))
    assert log_margin(tag + "dz (head)", _maxrel(dz3, want), 1e-4)
    assert log_margin(tag + "grad_bn_w (head)", _maxrel(gbw, sgx), 1e-4)
    assert log_margin(tag + "colsum (head)", _maxrel(colsum, want.sum(dim=0)), 1e-4)
    dw64 = torch.einsum("bvc,bvo->vco", _d(x_top), _d(ds_head)).reshape(nv, c * 3)
    dw_abs = torch.einsum("bvc,bvo->vco", _d(x_top).abs(), _d(ds_head).abs()).reshape(nv, c * 3)
    assert _within(tag + "dw_head", dw_head, dw64, (batch + 8) * 2.0 ** -24 * dw_abs)


def _spy_calls(monkeypatch):
    """The library entry points asked for from here on: the names that go through _lib.call, and -- marked "check:" -- every
    name whose status goes through _lib.check (those again, and the launches the layers issue themselves)."""
    calls = []
    real_call, real_check = _lib.call, _lib.check

    def call_spy(name, *args):
        calls.append(name)
        return real_call(name, *args)

    def check_spy(code, what):
        calls.append("check:" + what)
        return real_check(code, what)
    monkeypatch.setattr(_lib, "call", call_spy)
    monkeypatch.setattr(_lib, "check", check_spy)
    return calls


@pytest.mark.parametrize("mesh,batch", [("icosphere_162", 33), ("uv_sphere_482", 24)])
@pytest.mark.parametrize("relu", [False, True])
def test_the_wide_block_against_float64_and_against_the_separate_operators(gpu, mesh, batch, relu, monkeypatch):
    """The assertions of test_the_fused_block_against_float64_and_against_the_separate_operators (see there for why the ReLU
    chain's gradients are held in the L2 norm) at batches the wide launches serve."""
    nv, adj, csr = _mesh(mesh, gpu)
    tag = "wide block %s b%d relu=%d " % (mesh, batch, relu)
    torch.manual_seed(5)
    block = models.BatchMeshDeformationBlock(3 + 200, nv).to(gpu).train()
    with torch.no_grad():
        for i in range(1, 14):
            getattr(block, "bn%d" % i).weight.uniform_(0.5, 1.5)
            getattr(block, "bn%d" % i).bias.uniform_(-0.3, 0.3)
    twin = copy.deepcopy(block)
    feats = torch.randn(batch, nv, 3, device=gpu)
    pooled = torch.randn(batch, nv, 200, device=gpu)
    g_f, g_c = torch.randn(batch, nv, 192, device=gpu), torch.randn(batch, nv, 3, device=gpu)
    monkeypatch.setattr(deform, "relu", relu)

    def run(blk, fused):
        monkeypatch.setattr(deform, "enabled", fused)
        f, p = feats.clone().requires_grad_(True), pooled.clone().requires_grad_(True)
        assert deform.serves_wide(blk, f, p, csr) == fused and not deform.serves(blk, f, p, csr)
        out_f, coords = blk(f, p, adj)
        ((out_f * g_f).sum() + (coords * g_c).sum()).backward()
        return out_f, coords, f.grad, p.grad
    calls = _spy_calls(monkeypatch)
    out_f, coords, gf, gp = run(block, True)
    assert calls.count("geom_deform_layer_wide_fwd_f32") == 13 and calls.count("geom_deform_layer_wide_bwd_f32") == 13
    assert calls.count("geom_deform_pack_weights_zero_f32") == 1
    assert not [c for c in calls if "geom_vertex_bn_" in c or "geom_deform_chain" in c
                or c in ("geom_deform_layer_fwd_f32", "geom_deform_layer_bwd_f32")]
    f64, p64 = _d(feats).requires_grad_(True), _d(pooled).requires_grad_(True)
    e_f, e_c, params64 = _block64(block, f64, p64, adj, relu)
    ((e_f * _d(g_f)).sum() + (e_c * _d(g_c)).sum()).backward()
    assert log_margin(tag + "features", _maxrel(out_f, e_f), 2e-5) and log_margin(tag + "coords", _maxrel(coords, e_c), 2e-5)
    named = dict(block.named_parameters())
    pairs = [(n, p.grad, params64[n].grad) for n, p in named.items() if not n.startswith("bn14")]
    pairs += [("features", gf, f64.grad), ("pooled", gp, p64.grad)]
    assert all(named[n].grad is None for n in named if n.startswith("bn14"))
    sd = block.state_dict()
    assert int(sd["bn1.num_batches_tracked"]) == 1 and int(sd["bn13.num_batches_tracked"]) == 1
    assert int(sd["bn14.num_batches_tracked"]) == 0
    if not relu:
        bad = [name for name, got, want in pairs if not log_margin(tag + "grad " + name, _maxrel(got, want), 5e-5)]
        assert not bad, bad
        return
    ref_f, ref_c, rgf, rgp = run(twin, False)          # the separate operators on the same parameters
    assert log_margin(tag + "features vs separate", _maxrel(out_f, ref_f), 2e-5)
    assert log_margin(tag + "coords vs separate", _maxrel(coords, ref_c), 2e-5)
    bad = [name for name, got, want in pairs if not log_margin(tag + "grad " + name + " L2", _l2rel(got, want), 5e-3)]
    assert not bad, bad
    for i in range(1, 14):
        a, b = getattr(block, "bn%d" % i), getattr(twin, "bn%d" % i)
        assert log_margin(tag + "running_mean[%d] vs separate" % i, _maxrel(a.running_mean, b.running_mean), 1e-4)
        assert log_margin(tag + "running_var[%d] vs separate" % i, _maxrel(a.running_var, b.running_var), 1e-4)


def test_block192_reference_fixture_on_the_wide_route(gpu, monkeypatch):
    """Case ico162_b24 of tests/golden/block192.npz (the REFERENCE's BatchMeshDeformationBlock(195, V) run in float64) with the
    bars of test_block192_against_the_reference_fixture: 2e-5 forward, 1e-5 running statistics, 5e-5 for every gradient
    element and checksum; the wide launches are the ones issued; the stored eval forward afterwards."""
    case = "ico162_b24"
    g = block192_fixture(case)
    inp = block192_case(g)
    b, nv = int(g["batch"]), int(g["nv"])
    assert b == 24
    V, Fc = meshgen.icosphere(2)
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    a = adj.cpu().numpy()
    r, c = np.nonzero(a)
    assert np.array_equal(r, g["adj_rows"]) and np.array_equal(c, g["adj_cols"]) and np.array_equal(bits(a[r, c]), bits(g["adj_vals"]))
    csr = layers.adjacency_csr(adj)
    block = block192_parameters(models.BatchMeshDeformationBlock(195, nv), g).to(gpu).train()
    named = dict(block.named_parameters())
    to = lambda k: torch.from_numpy(inp[k]).to(gpu)          # noqa: E731
    feats, pooled = to("features").requires_grad_(True), to("pooled").requires_grad_(True)
    assert deform.serves_wide(block, feats, pooled, csr) and not deform.serves(block, feats, pooled, csr)
    monkeypatch.setattr(deform, "relu", bool(g["relu"]))
    calls = _spy_calls(monkeypatch)
    out_f, coords = block(feats, pooled, adj)
    ((out_f * to("g_features")).sum() + (coords * to("g_coords")).sum()).backward()
    assert calls.count("geom_deform_layer_wide_fwd_f32") == 13 and calls.count("geom_deform_layer_wide_bwd_f32") == 13
    assert not [c for c in calls if "geom_vertex_bn_" in c or "geom_deform_chain" in c]
    monkeypatch.setattr(deform, "relu", True)
    sd = block.state_dict()
    assert all(int(sd["bn%d.num_batches_tracked" % i]) == 1 for i in range(1, 14)) and int(sd["bn14.num_batches_tracked"]) == 0
    np64 = lambda t: t.detach().double().cpu().numpy()         # noqa: E731
    full = {"features": np64(out_f), "coords": np64(coords), "grad.features": np64(feats.grad), "grad.pooled": np64(pooled.grad),
            "running_mean": np.stack([np64(getattr(block, "bn%d" % i).running_mean) for i in range(1, 14)]),
            "running_var": np.stack([np64(getattr(block, "bn%d" % i).running_var) for i in range(1, 14)])}
    full.update({"grad." + k: np64(p.grad) for k, p in named.items() if not k.startswith("bn14")})
    if "eval.coords" in g:
        block.eval()
        with torch.no_grad():
            e_f, e_c = block(feats.detach(), pooled.detach(), adj)
        full.update({"eval.features": np64(e_f), "eval.coords": np64(e_c)})
    assert sorted(full) == list(g["ck_names"])
    stored = block192_stored(g, full)

    def maxrel(x, y):
        return float(np.abs(x - y).max()) / max(float(np.abs(y).max()), 1e-30)

    def tensors(key, x):          # (the 13 layers' stacked vectors are 13 tensors)
        if key in ("grad.gc_bias", "grad.bn_weight", "grad.bn_bias", "running_mean", "running_var"):
            return [("wide %s %s[layer %d]" % (case, key, i + 1), t) for i, t in enumerate(x)]
        return [("wide %s %s" % (case, key), x)]
    bad = []
    for key, got in stored.items():
        for (what, x), (_, y) in zip(tensors(key, got), tensors(key, g[key].astype(np.float64))):
            bar = 5e-5 if key.startswith("grad.") else 1e-5 if key.startswith("running") else 2e-5
            if not log_margin(what + " max-norm", maxrel(x, y), bar):
                bad.append("%s: %.2e of scale (bar %g)" % (what, maxrel(x, y), bar))
    for name, (want, scale) in zip(g["ck_names"], g["ck"]):
        name = str(name)
        bar = 1e-5 if name.startswith("running") else 2e-5 if not name.startswith("grad.") else 5e-5
        err = abs(weighted_checksum(name, full[name])[0] - want) / scale
        if not log_margin("wide %s checksum %s" % (case, name), err, bar):
            bad.append("checksum of %s: %.2e of its scale (bar %g)" % (name, err, bar))
    assert not bad, "; ".join(bad)


def test_the_wide_block_is_bit_reproducible_and_replays_inside_a_hip_graph(gpu):
    nv, adj, csr = _mesh("uv_sphere_482", gpu)
    torch.manual_seed(6)
    block = models.BatchMeshDeformationBlock(3 + 197, nv).to(gpu).train()
    feats = torch.randn(32, nv, 3, device=gpu, requires_grad=True)
    pooled = torch.randn(32, nv, 197, device=gpu, requires_grad=True)
    assert deform.serves_wide(block, feats, pooled, csr)
    params = list(block.parameters())
    kept = {}

    def rewind():      # the running statistics move with every step: every step starts where the first did
        for i in range(1, 14):
            getattr(block, "bn%d" % i).running_mean.zero_(), getattr(block, "bn%d" % i).running_var.fill_(1.0)

    def step():
        for p in params:
            p.grad = None
        feats.grad = pooled.grad = None
        f, c = block(feats, pooled, adj)
        (f.sum() + c.sum()).backward()
        kept["out"] = (f.detach(), c.detach())

    def results():
        return ([p.grad.clone() for p in params if p.grad is not None] + [feats.grad.clone(), pooled.grad.clone()]
                + [t.clone() for t in kept["out"]] + [getattr(block, "bn%d" % i).running_var.clone() for i in range(1, 14)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    runs = []
    with torch.cuda.stream(side):
        step()                      # (whatever is set up on a first call)
        for _ in range(2):
            rewind()
            step()
            runs.append(results())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))      # two eager steps: the same bits
    rewind()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        step()
    g.replay()
    torch.cuda.synchronize()
    replayed = results()
    assert len(replayed) == len(runs[0])
    for a, b in zip(runs[0], replayed):
        assert torch.equal(a, b)          # same launches, fixed reduction orders: bit-reproducible


def test_wide_routing(gpu, monkeypatch, tmp_path):
    nv, adj, csr = _mesh("icosphere_162", gpu)
    torch.manual_seed(12)
    block = models.BatchMeshDeformationBlock(200, nv).to(gpu).train()

    def inputs(b):
        return torch.randn(b, nv, 3, device=gpu, requires_grad=True), torch.randn(b, nv, 197, device=gpu)

    def runs_finite(blk, f, p):
        out_f, coords = blk(f, p, adj)
        if f.requires_grad and torch.is_grad_enabled():
            (out_f.sum() + coords.sum()).backward()
            assert torch.isfinite(f.grad).all()
        assert torch.isfinite(out_f).all() and torch.isfinite(coords).all()
    f24, p24 = inputs(24)
    assert deform.serves_wide(block, f24, p24, csr) and not deform.serves(block, f24, p24, csr)
    assert deform.serves_wide(block, *inputs(17), csr) and deform.serves_wide(block, *inputs(64), csr)
    f16, p16 = inputs(16)
    assert deform.serves(block, f16, p16, csr) and not deform.serves_wide(block, f16, p16, csr)      # the plain launches' ground
    runs_finite(block, f16, p16)
    f65, p65 = inputs(65)
    assert not deform.serves_wide(block, f65, p65, csr) and not deform.serves(block, f65, p65, csr)
    runs_finite(block, f65, p65)
    block.eval()
    assert not deform.serves_wide(block, f24, p24, csr)
    runs_finite(block, *inputs(24))
    block.train()
    with torch.no_grad():
        assert not deform.serves_wide(block, f24, p24, csr)
        runs_finite(block, f24, p24)
    synced = models.BatchMeshDeformationBlock(200, nv).to(gpu).train()
    for i in range(1, 15):
        getattr(synced, "bn%d" % i).sync_across_ranks = True
    assert deform.serves_wide(synced, f24, p24, csr)      # (no process group: nothing to synchronise with)
    import torch.distributed as dist
    monkeypatch.setenv("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:      # a one-rank group that takes the synchronised route (as tests/dist_step_worker.py does)
        monkeypatch.setattr(models.VertexBatchNorm, "_sync_single_rank_groups", True)
        assert synced.bn1._synchronised() and not deform.serves_wide(synced, f24, p24, csr)
        runs_finite(synced, *inputs(24))
        monkeypatch.setattr(models.VertexBatchNorm, "_sync_single_rank_groups", False)
    finally:
        dist.destroy_process_group()
    no_momentum = models.BatchMeshDeformationBlock(200, nv).to(gpu).train()
    no_momentum.bn7.momentum = None
    assert not deform.serves_wide(no_momentum, f24, p24, csr)
    monkeypatch.setattr(deform, "enabled", False)
    assert not deform.serves_wide(block, f24, p24, csr)
    runs_finite(block, *inputs(24))
    monkeypatch.setattr(deform, "enabled", True)
    monkeypatch.setattr(deform, "wide", False)
    assert not deform.serves_wide(block, f24, p24, csr)
    calls = _spy_calls(monkeypatch)
    runs_finite(block, *inputs(24))
    assert calls and not [c for c in calls if "wide" in c]
    monkeypatch.setattr(deform, "wide", True)
    assert deform.serves_wide(block, f24, p24, csr)
    del calls[:]
    runs_finite(block, *inputs(24))
    assert calls.count("geom_deform_layer_wide_fwd_f32") == 13 and calls.count("geom_deform_layer_wide_bwd_f32") == 13
