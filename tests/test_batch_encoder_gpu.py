"""The batched mesh encoder with frozen parameters on one launch per layer and direction (csrc/encoder_stack.hip,
geometrics_amd/encoder.py) and the latent loss, against the reference's float64 run (tests/golden/batch_mesh_encoder.npz,
made by tests/golden/make_batch_encoder.py).

The head takes its max over the vertices of un-activated values; the fixture's parameters are at the reference
initialiser's scale (gain 6), where the top-2 gap of that max is >= 1.3e-4 of scale -- at the default gain of
helpers.fill_parameters it is ~1e-7 and float32 flips arg-maxes at random.  The bars: values 2e-5 of scale (what the block
tests hold 13 layers to; <= gap / 4, so the arg-max cannot flip inside it), position gradients 4 x the distance of the
reference's OWN float32 run from its float64 run (the ratio block192_eval keeps), never above 1e-3."""
import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
CASES = ("ico162_b2", "uv482_b3")
VALUE_BAR = 2e-5
# (cin, cout) of a layer product; the launch in front of it transforms a cin-wide operand
PAIRS = [(3, 60), (60, 60), (120, 150), (210, 250), (250, 300), (300, 300), (300, 50)]


@pytest.fixture(scope="module")
def fx():
    return helpers.golden("batch_mesh_encoder")


def _case(fx, case):
    return {k[len(case) + 1:]: v for k, v in fx.items() if k.startswith(case + ".")}


_meshes = {}


def _mesh(name):
    """(template vertices, faces, dense normalised adjacency on the device, its CSR) of a fixture mesh, made once."""
    if name not in _meshes:
        from geometrics_amd import layers, meshgen, utils
        V, Fc = meshgen.uv_sphere() if name == "uv_sphere" else meshgen.icosphere(2)
        adj = utils.adj_init(torch.from_numpy(np.ascontiguousarray(Fc)).cuda())["adj"]
        _meshes[name] = (V, Fc, adj, layers.adjacency_csr(adj))
    return _meshes[name]


MESHES = [("icosphere_2", 2), ("uv_sphere", 3)]          # 324 and 1446 rows: a ragged last row tile; the uv sphere's two 33-entry pole rows


@pytest.fixture
def fused_on():
    from geometrics_amd import encoder
    was, encoder.enabled = encoder.enabled, True
    yield
    encoder.enabled = was


# ------------------------------------------------------------------------------------------------ the layer entry points ----
@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("mesh,batch", MESHES)
def test_layer_entry_forward(gpu, mesh, batch, cin, cout):
    from geometrics_amd import _lib, aggregation, encoder
    _, _, _, csr = _mesh(mesh)
    nv, rows = csr.nv, batch * csr.nv
    g = torch.Generator(device="cpu").manual_seed(100 * cin + cout + rows)
    s = torch.randn(rows, cin, generator=g).cuda()
    w = (torch.randn(cin, cout, generator=g) / cin ** 0.5).cuda()
    identity = cin == 3
    bias = None if identity else (0.3 * torch.randn(cin, generator=g)).cuda()
    k, act = (0, aggregation.ACT_NONE) if identity else (cin // 10, aggregation.ACT_ELU)
    x = torch.full((rows, cin), float("nan"), device="cuda")
    out = encoder.layer_forward(s, csr, k, bias, act, w, batch, nv, x_out=x)
    want_x = torch.empty_like(s)
    _lib.call("geom_zn_gcn_aggregate_fwd_f32", batch, nv, cin, k, csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(),
              s.data_ptr(), _lib.ptr(bias), act, want_x.data_ptr())
    assert torch.equal(x.view(torch.int32), want_x.view(torch.int32)), "the transformed operand differs from the aggregation's bits"
    if identity:
        assert torch.equal(x, s)
    else:
        assert float((want_x < 0).float().mean()) > 0.2            # both ELU branches
    x64, w64 = want_x.double().cpu(), w.double().cpu()
    helpers.rows_close(out.cpu(), x64 @ w64, x64.abs() @ w64.abs(), (cin + 8) * EPS, "fwd %s %d->%d" % (mesh, cin, cout))
    assert torch.equal(out, encoder.layer_forward(s, csr, k, bias, act, w, batch, nv))       # x_out = NULL: the same product


@pytest.mark.parametrize("cin,cout", [(3, 60), (120, 150), (250, 300)])
def test_layer_entry_without_a_tail_gives_the_any_shape_product_bits(gpu, cin, cout):
    """k = 0, no bias and no activation leave the launch a plain product, and geom_gemm_f32 is the other user of the same staged
    64 x 64 tile (csrc/mfma_tiles.h): at these widths (no split below K = 512, 32-deep stages in both, zero fill beyond K) an
    accumulator receives the same MFMA steps in the same order in both kernels -- the same bits, forward and backward, the
    backward also with its weight at a row pitch."""
    from geometrics_amd import _lib, aggregation, dense, encoder
    _, _, _, csr = _mesh("icosphere_2")
    batch, nv = 2, csr.nv
    rows = batch * nv
    gen = torch.Generator(device="cpu").manual_seed(1000 * cin + cout)
    s, g = torch.randn(rows, cin, generator=gen).cuda(), torch.randn(rows, cout, generator=gen).cuda()
    w = (torch.randn(cin, cout, generator=gen) / cin ** 0.5).cuda()
    none = aggregation.ACT_NONE

    def same_bits(a, b):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same_bits(encoder.layer_forward(s, csr, 0, None, none, w, batch, nv), dense.gemm(s, w))
    back = encoder.layer_backward(g, None, csr, 0, none, w, batch, nv)
    assert same_bits(back, dense.gemm(g, w, trans_b=True))
    frame = torch.full((cin, cout + 5), float("nan"), device="cuda")
    frame[:, 3:3 + cout] = w
    wp, out = frame[:, 3:3 + cout], torch.empty(rows, cin, device="cuda")
    _lib.call("geom_encoder_layer_bwd_f32", batch, nv, cout, 0, cin, None, None, None, g.data_ptr(), cout, None, cout, none,
              wp.data_ptr(), cout + 5, out.data_ptr(), cin, None, cout)
    assert same_bits(out, dense.gemm(g, wp, trans_b=True)) and same_bits(out, back)


@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("mesh,batch", MESHES)
def test_layer_entry_backward(gpu, mesh, batch, cin, cout):
    """The mirrored launch: a cout-wide gradient in, the cin-wide input gradient out (60 -> 3 is the last of a backward pass;
    50 -> 300 is the head's adjoint tail, no activation)."""
    from geometrics_amd import _lib, aggregation, encoder
    _, _, _, csr = _mesh(mesh)
    nv, rows = csr.nv, batch * csr.nv
    gen = torch.Generator(device="cpu").manual_seed(100 * cin + cout + rows + 1)
    g = torch.randn(rows, cout, generator=gen).cuda()
    w = (torch.randn(cin, cout, generator=gen) / cout ** 0.5).cuda()
    head = cout == 50
    act = aggregation.ACT_NONE if head else aggregation.ACT_ELU
    saved = None if head else torch.nn.functional.elu(torch.randn(rows, cout, generator=gen)).cuda()
    k = cout // 10
    t = torch.full((rows, cout), float("nan"), device="cuda")
    out = encoder.layer_backward(g, saved, csr, k, act, w, batch, nv, t_out=t)
    want_t = torch.empty_like(g)
    _lib.call("geom_zn_gcn_aggregate_bwd_f32", batch, nv, cout, k, csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(),
              csr.val_t.data_ptr(), g.data_ptr(), _lib.ptr(saved), act, want_t.data_ptr(), None, None)
    assert torch.equal(t.view(torch.int32), want_t.view(torch.int32)), "the transformed operand differs from the aggregation's bits"
    t64, w64 = want_t.double().cpu(), w.double().cpu().t()
    helpers.rows_close(out.cpu(), t64 @ w64, t64.abs() @ w64.abs(), (cout + 8) * EPS, "bwd %s %d->%d" % (mesh, cout, cin))
    assert torch.equal(out, encoder.layer_backward(g, saved, csr, k, act, w, batch, nv))


def test_layer_entry_pitched_views_touch_nothing_else(gpu):
    """Every matrix in a wider frame at an odd 4-byte offset: only the addressed elements are read (NaN around them) and
    written (the frame keeps its fill)."""
    from geometrics_amd import _lib, aggregation
    _, _, _, csr = _mesh("icosphere_2")
    b, nv, c, n, k = 2, csr.nv, 61, 67, 6
    rows = b * nv
    gen = torch.Generator(device="cpu").manual_seed(5)
    s_frame = torch.full((rows, 71), float("nan"), device="cuda")
    w_frame = torch.full((c, 75), float("nan"), device="cuda")
    s_frame[:, 3:3 + c] = torch.randn(rows, c, generator=gen).cuda()
    w_frame[:, 5:5 + n] = torch.randn(c, n, generator=gen).cuda()
    bias = torch.randn(c, generator=gen).cuda()
    o_frame = torch.full((rows, 73), 7.0, device="cuda")
    x_frame = torch.full((rows, 63), 7.0, device="cuda")
    s, w, out, x = s_frame[:, 3:3 + c], w_frame[:, 5:5 + n], o_frame[:, 1:1 + n], x_frame[:, 1:1 + c]
    _lib.call("geom_encoder_layer_fwd_f32", b, nv, c, k, n, csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(),
              s.data_ptr(), 71, bias.data_ptr(), aggregation.ACT_ELU, w.data_ptr(), 75, out.data_ptr(), 73, x.data_ptr(), 63)
    want_x = torch.empty(rows, c, device="cuda")
    _lib.call("geom_zn_gcn_aggregate_fwd_f32", b, nv, c, k, csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(),
              s.contiguous().data_ptr(), bias.data_ptr(), aggregation.ACT_ELU, want_x.data_ptr())
    assert torch.equal(x, want_x)
    x64, w64 = want_x.double().cpu(), w.double().cpu()
    helpers.rows_close(out.cpu(), x64 @ w64, x64.abs() @ w64.abs(), (c + 8) * EPS, "pitched forward")
    o_frame[:, 1:1 + n] = 7.0
    x_frame[:, 1:1 + c] = 7.0
    assert bool((o_frame == 7.0).all()) and bool((x_frame == 7.0).all())


# ---------------------------------------------------------------------------------------------------------- latent loss ----
def _loss64(pred, target, on, weight=.0005):
    return weight * (torch.mean(torch.abs(pred - target), dim=1) * on / (on.sum())).sum()           # GEOMetrics.py:167


@pytest.mark.parametrize("b,l,on", [(2, 50, (1, 1)), (3, 50, (1, 0, 1)), (300, 7, None), (1, 1, (2,))])
def test_latent_loss_against_float64(gpu, b, l, on):
    """Forward and gradient against the reference's expression in float64.  The loss is a sum of non-negative terms, each
    through l + b + a few fp32 roundings: (l + b + 8) eps relative; a gradient element is a product of five factors: 8 eps."""
    from geometrics_amd import utils
    gen = torch.Generator(device="cpu").manual_seed(b * 100 + l)
    pred, target = torch.randn(b, l, generator=gen), torch.randn(b, l, generator=gen)
    on_t = torch.tensor(on, dtype=torch.float32) if on is not None else (torch.rand(b, generator=gen) < 0.6).float()
    p = pred.cuda().requires_grad_(True)
    loss = utils.latent_loss(p, target.cuda(), on_t.cuda())
    assert loss.shape == ()
    (3.0 * loss).backward()
    p64 = pred.double().requires_grad_(True)
    want = _loss64(p64, target.double(), on_t.double())
    (3.0 * want).backward()
    assert helpers.log_margin("latent loss b=%d" % b, abs(float(loss) - float(want)) / float(want), (l + b + 8) * EPS)
    err = (p.grad.double().cpu() - p64.grad).abs()
    assert bool((err <= 8 * EPS * p64.grad.abs()).all())
    if on is not None and 0 in on:
        assert bool((p.grad[on.index(0)] == 0).all())


def test_latent_loss_with_no_latent_in_the_batch_is_exactly_zero(gpu):
    from geometrics_amd import utils
    p = torch.randn(4, 50, device="cuda").requires_grad_(True)
    loss = utils.latent_loss(p, torch.randn(4, 50, device="cuda"), torch.zeros(4, device="cuda"))
    loss.backward()
    assert float(loss) == 0.0 and bool((p.grad == 0).all())            # (no NaN: NaN == 0 is false)
    # on_latent as the loader hands it over (any dtype, [B] or [B,1])
    on = torch.tensor([[1], [0], [1], [1]], dtype=torch.float64, device="cuda")
    assert float(utils.latent_loss(p, p.detach() + 1.0, on)) == pytest.approx(.0005, rel=1e-6)


# ------------------------------------------------------------------------------------------------------------ end to end ----
def _inputs(c):
    V, Fc, adj, _ = _mesh(str(c["mesh"]))
    seed, batch = int(c["seed"]), int(c["batch"])
    noise = np.random.default_rng([seed, 0]).standard_normal((batch,) + V.shape)
    pos = (V[None].astype(np.float64) + 0.03 * noise).astype(np.float32)
    assert float(pos.astype(np.float64).sum()) == float(c["in_ck"])
    return torch.from_numpy(pos).cuda(), adj


def _encoder(c, frozen=True):
    from geometrics_amd import models
    enc = helpers.fill_parameters(models.BatchMeshEncoder(50), int(c["seed"]), gain=6.0).cuda()
    return enc.requires_grad_(not frozen)


def _of_scale(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def _check_case(case, c, enc, route):
    """Every bar of a case on the route the encoder takes."""
    from geometrics_amd import utils
    pos, adj = _inputs(c)
    p = pos.clone().requires_grad_(True)
    v = enc.pre_max(p, adj)
    assert enc.last_route == route
    lat = enc(p, adj)
    assert enc.last_route == route
    ok = []
    # values: sampled rows and the weighted checksum of v, the latents, the arg-max vertices
    v64 = v.detach().double().cpu().numpy()
    scale_v = float(c["v_scale"])
    ok.append(helpers.log_margin("%s %s v rows" % (case, route),
                                 float(np.abs(v64[c["rows_b"], c["rows_v"]] - c["v_rows"]).max()) / scale_v, VALUE_BAR))
    ck = helpers.weighted_checksum("v", v64)
    mass = float(np.abs(helpers.checksum_weights("v", v64.shape)).sum())      # every element within the bar moves the sum by this
    ok.append(helpers.log_margin("%s %s v checksum" % (case, route), abs(ck[0] - c["v_ck"][0]) / (scale_v * mass), VALUE_BAR))
    ok.append(helpers.log_margin("%s %s latents" % (case, route), _of_scale(lat.detach().cpu().numpy(), c["latents"]), VALUE_BAR))
    assert np.array_equal(v.detach().argmax(dim=1).cpu().numpy(), c["argmax"])
    if route == "fused":                                             # (its launches are bit-reproducible: the two calls agree)
        assert torch.equal(lat.detach(), v.detach().max(dim=1)[0])
    # the latent loss and its gradient; the gradient of sum(v * G)
    target, on = torch.from_numpy(c["target"]).cuda(), torch.from_numpy(c["on_latent"]).cuda()
    loss = utils.latent_loss(lat, target, on, float(c["weight"]))
    scale_l = float(np.abs(c["latents"]).max())
    ok.append(helpers.log_margin("%s %s loss" % (case, route), abs(float(loss) - float(c["loss"])) / (float(c["weight"]) * scale_l),
                                 VALUE_BAR))
    (g_loss,) = torch.autograd.grad(loss, p)
    G = torch.from_numpy(helpers.seeded_input([int(c["seed"]), 2], tuple(v.shape))).cuda()
    (g_v,) = torch.autograd.grad((v * G).sum(), p)
    for name, got in (("grad_latent_loss", g_loss), ("grad_vG", g_v)):
        bar = min(4.0 * float(c["float32." + name]), 1e-3)
        ok.append(helpers.log_margin("%s %s %s" % (case, route, name), _of_scale(got.cpu().numpy(), c[name]), bar))
    for m in np.nonzero(c["on_latent"] == 0)[0]:
        assert bool((g_loss[int(m)] == 0).all())                     # a mesh without a latent receives exactly nothing
    assert all(ok), "a margin is above its bar: run with GEOM_MARGIN_LOG set"


@pytest.mark.parametrize("case", CASES)
def test_frozen_encoder_end_to_end_on_the_fused_route(gpu, fx, fused_on, case):
    c = _case(fx, case)
    _check_case(case, c, _encoder(c), "fused")


@pytest.mark.parametrize("case", CASES)
def test_switch_off_takes_the_separate_operators_to_the_same_bars(gpu, fx, case):
    from geometrics_amd import encoder
    c = _case(fx, case)
    was, encoder.enabled = encoder.enabled, False
    try:
        _check_case(case, c, _encoder(c), "separate")
    finally:
        encoder.enabled = was


@pytest.mark.parametrize("case", CASES)
def test_trainable_parameters_take_the_separate_operators(gpu, fx, fused_on, case):
    """Parameters that require grad: the plain composition of the layers, parameter gradients included (of sum(v * G))."""
    c = _case(fx, case)
    enc = _encoder(c, frozen=False)
    pos, adj = _inputs(c)
    v = enc.pre_max(pos, adj)
    assert enc.last_route == "separate"
    G = torch.from_numpy(helpers.seeded_input([int(c["seed"]), 2], tuple(v.shape))).cuda()
    (v * G).sum().backward()
    rows = torch.from_numpy(c["w_rows"].astype(np.int64))
    ok = []
    for name, got in (("h1.weight", enc.h1.weight.grad), ("h24.weight", enc.h24.weight.grad),
                      ("reduce.weight_Ws.0", enc.reduce.weight_Ws[0].grad[rows.cuda()])):
        ok.append(helpers.log_margin("%s grad.%s" % (case, name), _of_scale(got.cpu().numpy(), c["grad." + name]), 1e-3))
    assert all(ok)


def test_fused_forward_and_backward_replay_from_a_graph(gpu, fx, fused_on):
    """Forward + latent loss + backward of the fused route captured on one stream, replayed on positions the capture never
    saw: the bits of the eager call."""
    from geometrics_amd import utils
    c = _case(fx, "ico162_b2")
    enc = _encoder(c)
    pos, adj = _inputs(c)
    target, on = torch.from_numpy(c["target"]).cuda(), torch.from_numpy(c["on_latent"]).cuda()

    def step(p):
        lat = enc(p, adj)
        (grad,) = torch.autograd.grad(utils.latent_loss(lat, target, on), p)
        return lat.detach(), grad

    static = pos.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)                                                 # (warm-up: the CSR, the library, the allocator)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lat_g, grad_g = step(static)
    assert enc.last_route == "fused"
    other = pos.flip(0) * 1.01 + 0.002
    with torch.no_grad():
        static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    lat_e, grad_e = step(other.clone().requires_grad_(True))
    assert torch.equal(lat_g, lat_e) and torch.equal(grad_g, grad_e)
    assert not torch.equal(lat_e, step(pos.clone().requires_grad_(True))[0])      # (the replay did see other positions)
