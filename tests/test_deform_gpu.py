"""-m gpu: the hidden layers of the mesh deformation block as one launch per layer and direction (csrc/deform_block.hip,
geometrics_amd/deform.py; reference models.py:237-297 on layers.py:107-116).

* a single forward / backward launch against the separate operators it replaces (aggregation bits identical; the per-vertex
  BatchNorm and the products within fp32 summation order of a float64 evaluation);
* the whole block (13 fused hidden layers) against a FLOAT64 restatement of the reference block on the host: features,
  coordinates, running statistics, every parameter gradient and both input gradients;
* the same against the block on the separate operators (`deform.enabled = False`), batch 16 on the 482-vertex template with its
  two 33-entry poles (table + CSR tail) and batch 5 on a pole-free icosphere (rows beyond the batch are zero rows of the tile);
* the step inside a HIP graph; shapes the launches do not serve fall back to the separate operators;
* the thirteen launches of a direction as ONE (a vertex's workgroup waits for its neighbours' rows inside the launch): bit for
  bit the layer-by-layer launches; only the stream that owns a device's chain launches issues them; a mesh whose workgroups are
  not all resident at once takes the layer-by-layer launches;
* the block at width 192 against the reference's own block run in float64 (tests/golden/block192.npz): the chain launch,
  the smooth chain, per-layer BatchNorm settings, the batch > 16 fall-back and the eval-mode forward;
* a directed adjacency takes the launches per layer (never the chain), a block for another vertex count raises on the host."""
import numpy as np
import pytest
import torch

from geometrics_amd import deform, layers, meshgen, models, utils
from helpers import (BLOCK192_CASES, bits, block192_case, block192_fixture, block192_parameters, block192_stored, log_margin,
                     weighted_checksum)
from helpers import bn64 as _bn64, block64 as _block64

pytestmark = pytest.mark.gpu


def _mesh(name, gpu):
    V, Fc = meshgen.uv_sphere() if name == "uv_sphere_482" else meshgen.icosphere(2)
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    return V.shape[0], adj, layers.adjacency_csr(adj)


def _maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("mesh,batch", [("uv_sphere_482", 16), ("icosphere_162", 5)])
def test_one_forward_launch_against_the_separate_operators(gpu, mesh, batch):
    nv, adj, csr = _mesh(mesh, gpu)
    torch.manual_seed(3)
    c = 192
    s = torch.randn(batch, nv, c, device=gpu)
    bias = torch.randn(c, device=gpu) * 0.1
    gamma, beta = torch.rand(nv, device=gpu) + 0.5, torch.randn(nv, device=gpu) * 0.2
    res = torch.randn(batch, nv, c, device=gpu)
    w = torch.randn(c, c, device=gpu) / 14
    rm, rv = torch.zeros(nv, device=gpu), torch.ones(nv, device=gpu)
    z, x, s_next = (torch.empty_like(s) for _ in range(3))
    mean, invstd = torch.empty(nv, device=gpu), torch.empty(nv, device=gpu)
    packed, _ = deform.pack_weights([w])
    deform.layer_forward(s, bias, csr, gamma, beta, rm, rv, True, 0.1, 1e-5, True, res, 0.5, z, x, mean, invstd, w_next=packed[0], s_out=s_next)
    # aggregation: the bits of the stand-alone operator
    z_ref = layers.zero_n_aggregate(s, adj, bias, 64, None)
    assert torch.equal(z, z_ref)
    # BatchNorm + ReLU + residual average, and the product, against float64
    y64, m64, v64 = _bn64(z.double().cpu(), gamma.double().cpu(), beta.double().cpu(), 1e-5)
    x64 = (res.double().cpu() + torch.relu(y64)) * 0.5
    assert _maxrel(x, x64) <= 2e-6
    assert _maxrel(mean, m64) <= 1e-5 and _maxrel(invstd, 1.0 / torch.sqrt(v64 + 1e-5)) <= 1e-5
    n = batch * c
    assert _maxrel(rm, 0.1 * m64) <= 1e-5 and _maxrel(rv, 0.9 + 0.1 * v64 * n / (n - 1)) <= 1e-5
    s64 = x.double().cpu() @ w.double().cpu()
    bound = (c + 8) * 2.0 ** -24 * (x.double().cpu().abs() @ w.double().cpu().abs())
    assert bool(((s_next.double().cpu() - s64).abs() <= bound + 1e-30).all())
    # no product: the last hidden layer
    x2 = torch.empty_like(s)
    deform.layer_forward(s, bias, csr, gamma, beta, rm.clone(), rv.clone(), True, 0.1, 1e-5, True, None, 0.5, None, x2, mean, invstd)
    assert _maxrel(x2, torch.relu(y64)) <= 2e-6


@pytest.mark.parametrize("mesh,batch", [("uv_sphere_482", 16), ("icosphere_162", 5)])
def test_one_backward_launch_against_the_separate_operators(gpu, mesh, batch):
    nv, adj, csr = _mesh(mesh, gpu)
    torch.manual_seed(4)
    c = 192
    shape = (batch, nv, c)
    dz_up, z, g2 = (torch.randn(*shape, device=gpu) for _ in range(3))
    wt = torch.randn(c, c, device=gpu) / 14
    gamma, beta = torch.rand(nv, device=gpu) + 0.5, torch.randn(nv, device=gpu) * 0.2
    z64 = z.double().cpu()
    mean64 = z64.mean(dim=(0, 2))
    var64 = ((z64 - mean64.view(1, -1, 1)) ** 2).mean(dim=(0, 2))
    mean, invstd = mean64.float().to(gpu), (1.0 / torch.sqrt(var64 + 1e-5)).float().to(gpu)
    ds, dz, gres = (torch.empty(*shape, device=gpu) for _ in range(3))
    gbw, gbb = torch.empty(nv, device=gpu), torch.empty(nv, device=gpu)
    colsum = torch.empty(nv, c, device=gpu)
    _, packed_t = deform.pack_weights([wt.t().contiguous()])      # the launch reads the layer's weight transposed, packed
    deform.layer_backward(shape, csr, z, gamma, beta, mean, invstd, True, True, 0.5, dz, gbw, gbb, dz_up=dz_up, ds_up=ds, wt_up=packed_t[0],
                          g2=g2, grad_res=gres, colsum=colsum)
    ds_ref, _ = layers.aggregate_backward(dz_up, csr, 64, layers._ACT_NONE, None, None, False)
    assert torch.equal(ds, ds_ref)
    # float64 from here: dX = dS . W^T (wt IS the transposed weight), + g2, residual scale, ReLU mask, BatchNorm backward
    gx = (ds.double().cpu() @ wt.double().cpu() + g2.double().cpu()) * 0.5
    assert _maxrel(gres, gx) <= 2e-6
    m, i = mean.double().cpu().view(1, -1, 1), invstd.double().cpu().view(1, -1, 1)
    xh = (z64 - m) * i
    ga, be = gamma.double().cpu().view(1, -1, 1), beta.double().cpu().view(1, -1, 1)
    # (an element whose normalised value sits within rounding of the ReLU kink may fall on either side in float64: the mask is
    # formed in fp32, operation by operation as the kernel forms it -- and as the forward launch formed its ReLU)
    on = ((((z - mean.view(1, -1, 1)) * invstd.view(1, -1, 1)) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)) > 0).cpu()
    gy = torch.where(on, gx, torch.zeros_like(gx))
    sg, sgx = gy.sum(dim=(0, 2)), (gy * xh).sum(dim=(0, 2))
    n = batch * c
    dz64 = ga * i * (gy - sg.view(1, -1, 1) / n - xh * sgx.view(1, -1, 1) / n)
    assert _maxrel(gbb, sg) <= 1e-4 and _maxrel(gbw, sgx) <= 1e-4
    assert _maxrel(dz, dz64) <= 1e-4
    assert _maxrel(colsum, dz64.sum(dim=0)) <= 1e-4
    # no product: the gradient of the output is read from memory (+ the second one)
    g = torch.randn(*shape, device=gpu)
    dz2 = torch.empty(*shape, device=gpu)
    deform.layer_backward(shape, csr, z, gamma, beta, mean, invstd, True, False, 0.5, dz2, gbw, gbb, g=g, g2=g2)
    gy = torch.where(on, (g + g2).double().cpu(), torch.zeros_like(gx))
    sg, sgx = gy.sum(dim=(0, 2)), (gy * xh).sum(dim=(0, 2))
    assert _maxrel(dz2, ga * i * (gy - sg.view(1, -1, 1) / n - xh * sgx.view(1, -1, 1) / n)) <= 1e-4


def _l2rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


@pytest.mark.parametrize("mesh,batch", [("uv_sphere_482", 16), ("icosphere_162", 5)])
@pytest.mark.parametrize("relu", [False, True])
def test_the_fused_block_against_float64_and_against_the_separate_operators(gpu, mesh, batch, relu):
    """relu=False (deform.relu, tests only): the chain without its ReLUs is smooth, and EVERY gradient -- 13 fused backward
    launches deep -- is held to a max-norm bound against float64.  relu=True: the block as the reference runs it; a
    pre-activation within rounding of zero falls on either side in any two fp32 evaluations (expected: about one element in
    the block's 19 M per pass) and switches one unit's term, which moves single entries of a gradient by 1e-3 .. 1e-2 of its
    scale whatever the implementation -- so there the gradients are held in the L2 norm (a wrong mask, a dropped residual
    or a transposed tile is an O(1) error in it; one switched unit is ~1e-3), the forward in max-norm as before."""
    import copy
    nv, adj, csr = _mesh(mesh, gpu)
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

    def run(blk, fused):
        deform.enabled, deform.relu = fused, relu
        try:
            f, p = feats.clone().requires_grad_(True), pooled.clone().requires_grad_(True)
            assert deform.serves(blk, f, p, csr) == fused
            out_f, coords = blk(f, p, adj)
            ((out_f * g_f).sum() + (coords * g_c).sum()).backward()
        finally:
            deform.enabled, deform.relu = True, True
        return out_f, coords, f.grad, p.grad
    out_f, coords, gf, gp = run(block, True)
    f64, p64 = feats.double().cpu().requires_grad_(True), pooled.double().cpu().requires_grad_(True)
    e_f, e_c, params64 = _block64(block, f64, p64, adj, relu)
    ((e_f * g_f.double().cpu()).sum() + (e_c * g_c.double().cpu()).sum()).backward()
    # forward: 2e-5 of scale against float64 (the bar of the reference-fixture test of the block)
    assert _maxrel(out_f, e_f) <= 2e-5 and _maxrel(coords, e_c) <= 2e-5
    named = dict(block.named_parameters())
    pairs = [(n, p.grad, params64[n].grad) for n, p in named.items() if not n.startswith("bn14")]
    pairs += [("features", gf, f64.grad), ("pooled", gp, p64.grad)]
    assert all(named[n].grad is None for n in named if n.startswith("bn14"))
    if not relu:
        for name, got, want in pairs:
            assert _maxrel(got, want) <= 5e-5, "%s: %.2e of scale from float64" % (name, _maxrel(got, want))
        return
    ref_f, ref_c, rgf, rgp = run(twin, False)          # the separate operators on the same parameters
    assert _maxrel(out_f, ref_f) <= 2e-5 and _maxrel(coords, ref_c) <= 2e-5
    for name, got, want in pairs:
        assert _l2rel(got, want) <= 5e-3, "%s: %.2e from float64 in the L2 norm" % (name, _l2rel(got, want))
    for i in range(1, 14):
        a, b = getattr(block, "bn%d" % i), getattr(twin, "bn%d" % i)
        assert _maxrel(a.running_mean, b.running_mean) <= 1e-4 and _maxrel(a.running_var, b.running_var) <= 1e-4
    sd = block.state_dict()
    assert int(sd["bn1.num_batches_tracked"]) == 1 and int(sd["bn14.num_batches_tracked"]) == 0


def test_the_fused_block_replays_inside_a_hip_graph(gpu):
    nv, adj, csr = _mesh("uv_sphere_482", gpu)
    torch.manual_seed(6)
    block = models.BatchMeshDeformationBlock(3 + 197, nv).to(gpu).train()
    feats = torch.randn(16, nv, 3, device=gpu, requires_grad=True)
    pooled = torch.randn(16, nv, 197, device=gpu, requires_grad=True)
    params = list(block.parameters())

    def step():
        for p in params:
            p.grad = None
        feats.grad = pooled.grad = None
        f, c = block(feats, pooled, adj)
        (f.sum() + c.sum()).backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [p.grad.clone() for p in params if p.grad is not None] + [feats.grad.clone()]
    for i in range(1, 14):      # the running statistics move with every step: rewind so that the replay starts where the eager step did
        getattr(block, "bn%d" % i).running_mean.zero_(), getattr(block, "bn%d" % i).running_var.fill_(1.0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        step()
    g.replay()
    torch.cuda.synchronize()
    replayed = [p.grad for p in params if p.grad is not None] + [feats.grad]
    assert len(eager) == len(replayed)
    for a, b in zip(eager, replayed):
        assert torch.equal(a, b)          # same launches, fixed reduction orders: bit-reproducible


def test_shapes_the_launches_do_not_serve_take_the_separate_operators(gpu):
    nv, adj, csr = _mesh("icosphere_162", gpu)
    block = models.BatchMeshDeformationBlock(200, nv).to(gpu).train()
    narrow = models.BatchMeshDeformationBlock(200, nv, hidden=48).to(gpu).train()
    f, p = torch.randn(4, nv, 3, device=gpu), torch.randn(4, nv, 197, device=gpu)
    assert deform.serves(block, f, p, csr)
    assert not deform.serves(narrow, f, p, csr)                                        # another width
    assert not deform.serves(block, torch.randn(17, nv, 3, device=gpu), torch.randn(17, nv, 197, device=gpu), csr)   # more than one tile of meshes
    block.eval()
    assert not deform.serves(block, f, p, csr)                                         # running statistics: the library route
    with torch.no_grad():
        out_f, coords = block(f, p, adj)
    assert out_f.shape == (4, nv, 192) and coords.shape == (4, nv, 3)
    block.train()
    big = torch.randn(17, nv, 3, device=gpu, requires_grad=True)
    out_f, coords = block(big, torch.randn(17, nv, 197, device=gpu), adj)
    (out_f.sum() + coords.sum()).backward()
    assert torch.isfinite(big.grad).all()


# What a training forward + backward of the block issues on the separate operators (`deform.enabled = False`): the library entry
# points that go through _lib.call, in order; every entry point whose status goes through _lib.check (those, and the launches the
# layers issue themselves); and per VertexBatchNorm call (layer, residual given, tap).  Recorded ONCE, from the block as it was when
# its layer pairs were written out by hand; the loop over deform.SCHEDULE has to reproduce all three exactly.
SEPARATE_OPERATOR_CALLS = """
geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32
geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32
geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32 geom_vertex_bn_fwd_f32 geom_gemm_f32 geom_gemm_f32 geom_vertex_bn_bwd_f32
geom_vertex_bn_bwd_f32 geom_vertex_bn_bwd_f32 geom_vertex_bn_bwd_f32 geom_vertex_bn_bwd_f32 geom_vertex_bn_bwd_f32
geom_vertex_bn_bwd_f32 geom_vertex_bn_bwd_f32 geom_vertex_bn_bwd_f32 geom_vertex_bn_bwd_f32 geom_vertex_bn_bwd_f32
geom_vertex_bn_bwd_f32 geom_vertex_bn_bwd_f32
""".split()
SEPARATE_OPERATOR_CHECKS = """
geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32 geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32
geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32 geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32
geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32 geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32
geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32 geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32
geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32 geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32
geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32 geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32
geom_zn_gcn_aggregate_ell_fwd_f32 geom_vertex_bn_fwd_f32 geom_gemm_f32 geom_zn_gcn_aggregate_ell_fwd_f32
geom_zn_gcn_aggregate_ell_bwd_f32 geom_gemm_f32 geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32
geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32 geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32
geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32 geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32
geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32 geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32
geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32 geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32
geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32 geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32
geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32 geom_vertex_bn_bwd_f32 geom_zn_gcn_aggregate_ell_bwd_f32
""".split()
SEPARATE_OPERATOR_BATCHNORMS = [(1, False, False), (2, True, True), (3, False, False), (4, True, True), (5, False, False),
                                (6, True, True), (7, False, False), (8, True, True), (9, False, False), (10, True, True),
                                (11, False, False), (12, True, True), (13, True, True)]


def test_the_separate_operators_issue_what_they_issued(gpu, monkeypatch):
    from geometrics_amd import _lib
    nv, adj, csr = _mesh("icosphere_162", gpu)
    torch.manual_seed(11)
    block = models.BatchMeshDeformationBlock(200, nv).to(gpu).train()
    f = torch.randn(4, nv, 3, device=gpu, requires_grad=True)
    p = torch.randn(4, nv, 197, device=gpu, requires_grad=True)
    monkeypatch.setattr(deform, "enabled", False)

    def step():
        out_f, coords = block(f, p, adj)
        (out_f.sum() + coords.sum()).backward()
        torch.cuda.synchronize()
    step()                                   # (whatever is set up on a first call is not part of the sequence)
    calls, checks, norms = [], [], []
    real_call, real_check, real_bn = _lib.call, _lib.check, models.VertexBatchNorm.forward
    layer_of = {getattr(block, "bn%d" % i): i for i in range(1, 15)}

    def call_spy(name, *args):
        calls.append(name)
        return real_call(name, *args)

    def check_spy(code, what):
        checks.append(what)
        return real_check(code, what)

    def bn_spy(self, x, relu=False, residual=None, scale=0.5, tap=False):
        norms.append((layer_of[self], residual is not None, bool(tap)))
        return real_bn(self, x, relu=relu, residual=residual, scale=scale, tap=tap)
    monkeypatch.setattr(_lib, "call", call_spy)
    monkeypatch.setattr(_lib, "check", check_spy)
    monkeypatch.setattr(models.VertexBatchNorm, "forward", bn_spy)
    step()
    monkeypatch.undo()
    assert norms == SEPARATE_OPERATOR_BATCHNORMS
    assert checks == SEPARATE_OPERATOR_CHECKS
    assert calls == SEPARATE_OPERATOR_CALLS


def test_packed_weight_slices_hold_the_matrix_and_its_transpose(gpu):
    """geom_deform_pack_weights_f32: [wave][e / 4][lane][e % 4] with element e = (4 jp + c) * 3 + u of lane (x, g) =
    W[48 g + 4 jp + c][48 wave + 3 x + u] (and the same of W^T): a permutation of the matrix, checked index by index."""
    torch.manual_seed(8)
    ws = [torch.randn(1, 192, 192, device=gpu), torch.randn(192, 192, device=gpu)]
    fwd, bwd = deform.pack_weights(ws)
    r = np.arange(192 * 192)
    wave, rem = r // 9216, r % 9216
    i, lane, t = rem >> 8, (rem & 255) >> 2, rem & 3
    e = 4 * i + t
    jp, c, u = e // 12, (e // 3) & 3, e % 3
    g, x = lane >> 4, lane & 15
    k, col = 48 * g + 4 * jp + c, 48 * wave + 3 * x + u
    for n, w in enumerate(ws):
        m = w.reshape(192, 192).cpu().numpy()
        assert np.array_equal(fwd[n].cpu().numpy(), m[k, col]) and np.array_equal(bwd[n].cpu().numpy(), m[col, k])


def test_block_input_assembled_in_place_equals_the_concatenations(gpu):
    """The driver builds a block's input as cat(positions, cat(previous features, pooled)) (GEOMetrics.py:123-129, models.py:241).
    With `utils.batched_pooling(..., headroom=3 + 192)` + `utils.concat_features` the pooled features are written straight into
    the wide buffer, the fronts are copied into its free columns, and in the backward pass the pooling and the previous layer
    read their column slices of the ONE input gradient in place (row pitch 1155).  Against the same computation with plain
    torch.cat: features, coordinates and every gradient (maps, positions, previous features, parameters) bit for bit."""
    import copy
    from geometrics_amd import ops
    nv, adj, csr = _mesh("uv_sphere_482", gpu)
    torch.manual_seed(14)
    b = 16
    block = models.BatchMeshDeformationBlock(3 + 192 + 96, nv).to(gpu).train()
    twin = copy.deepcopy(block)
    maps = [torch.randn(b, c, d, d, device=gpu) for c, d in ((64, 14), (32, 7))]
    pos = (torch.from_numpy(meshgen.uv_sphere()[0]).to(gpu).unsqueeze(0) + 0.02 * torch.randn(b, nv, 3, device=gpu))
    prev = torch.randn(b, nv, 192, device=gpu)
    img = torch.tensor([[30.0 + 7 * i, 20.0, 1.2] for i in range(b)], device=gpu)
    g_f, g_c = torch.randn(b, nv, 192, device=gpu), torch.randn(b, nv, 3, device=gpu)

    def run(blk, in_place, fronts=False):
        ms = [m.clone().requires_grad_(True) for m in maps]
        p, f_prev = pos.clone().requires_grad_(True), prev.clone().requires_grad_(True)
        pooled = utils.batched_pooling(ms, p, img, headroom=3 + 192 if in_place else 0, fronts=(p, f_prev) if fronts else None)
        if fronts:      # the pooling launch placed both: the concatenations below copy nothing
            rec = ops.wide_buffer_of(pooled)
            buf = rec.buf
            assert buf is not None and rec.holds(0, p) and rec.holds(3, f_prev)
            assert torch.equal(buf[..., :3], p.detach()) and torch.equal(buf[..., 3:195], f_prev.detach())
        assert (ops.headroom_of(pooled) == 195) == in_place
        f = utils.concat_features(f_prev, pooled) if in_place else torch.cat((f_prev, pooled), dim=-1)
        assert f.shape == (b, nv, 192 + 96) and (ops.headroom_of(f) == 3) == in_place
        out_f, coords = blk(p, f, adj)
        ((out_f * g_f).sum() + (coords * g_c).sum()).backward()
        return [out_f.detach(), coords.detach(), p.grad, f_prev.grad] + [m.grad for m in ms] + [q.grad for q in blk.parameters() if q.grad is not None]
    want = run(twin, False)
    for fronts in (False, True):     # (True: positions and previous features copied into place by the pooling launch itself)
        got = run(copy.deepcopy(twin), True, fronts)
        assert len(got) == len(want) and len(got) >= 55
        for i, (a, w) in enumerate(zip(got, want)):
            if i in (4, 5):     # the maps' gradients: per-texel lists are filled in ticket order (same terms, fp32 order may differ: DESIGN 5)
                assert float((a - w).abs().max()) <= 1e-5 * float(w.abs().max())
            else:
                assert torch.equal(a, w), i
    with pytest.raises(RuntimeError):
        utils.batched_pooling([m.clone() for m in maps], pos, img, headroom=10, fronts=(pos,))      # widths must add up
    # pooling alone: the pitched forward and a pitched upstream gradient give the plain call's bits
    ms = [m.clone().requires_grad_(True) for m in maps]
    p = pos.clone().requires_grad_(True)
    wide = utils.batched_pooling(ms, p, img, headroom=5)
    plain = utils.batched_pooling([m.detach() for m in ms], p.detach(), img)
    assert torch.equal(wide, plain) and not wide.is_contiguous()
    g_wide = torch.randn(b, nv, 5 + 96, device=gpu)
    wide.backward(g_wide[..., 5:])
    ms2 = [m.clone().requires_grad_(True) for m in maps]
    p2 = pos.clone().requires_grad_(True)
    utils.batched_pooling(ms2, p2, img).backward(g_wide[..., 5:].contiguous())
    assert torch.equal(p.grad, p2.grad)
    assert all(float((x.grad - y.grad).abs().max()) <= 1e-5 * float(y.grad.abs().max()) for x, y in zip(ms, ms2))


def test_a_front_placed_by_the_pooling_launch_is_not_mistaken_for_the_next_tensor_at_its_address(gpu):
    """A front the pooling launch copied into the wide buffer is remembered by its memory; once that tensor is dropped, the
    allocator hands its block to the next tensor of the same shape (at version 0, as the old one was).  The concatenation
    must then copy the NEW tensor's columns -- the record holds the placed front's memory, so the address cannot come back
    while the wide buffer lives.  Values only: whether the allocator would have reused the block is not this test's business."""
    torch.manual_seed(15)
    maps = [torch.randn(2, 4, 8, 8, device=gpu), torch.randn(2, 4, 4, 4, device=gpu)]
    cams = torch.tensor([[30.0, 20.0, 1.2], [37.0, 20.0, 1.2]], device=gpu)
    pos = torch.randn(2, 12, 3, device=gpu)
    feat = torch.randn(2, 12, 5, device=gpu)
    pooled = utils.batched_pooling(maps, pos, cams, headroom=8, fronts=(pos, feat))
    del feat
    feat2 = torch.randn(2, 12, 5, device=gpu)
    out = utils.concat_features(feat2, pooled)
    plain = utils.batched_pooling(maps, pos, cams)
    assert out.shape == (2, 12, 13)
    assert torch.equal(out[..., :5], feat2)
    assert torch.equal(out[..., 5:], plain)
    # the block's own concatenation (models._InputTap) with the 3-column front
    front = torch.randn(2, 12, 3, device=gpu)
    pooled = utils.batched_pooling(maps, pos, cams, headroom=3, fronts=(front,))
    del front
    front2 = torch.randn(2, 12, 3, device=gpu)
    full, lead = models._InputTap.apply(front2, pooled, 3)
    assert full.shape == (2, 12, 11)
    assert torch.equal(full[..., :3], front2) and torch.equal(lead, front2)
    assert torch.equal(full[..., 3:], plain)


def _block_step(block, feats, pooled, adj):
    for p in block.parameters():
        p.grad = None
    feats.grad = pooled.grad = None
    for i in range(1, 14):
        getattr(block, "bn%d" % i).running_mean.zero_(), getattr(block, "bn%d" % i).running_var.fill_(1.0)
    f, c = block(feats, pooled, adj)
    (f * torch.linspace(-1, 1, f.shape[-1], device=f.device)).sum().add((c * c).sum()).backward()
    out = [f.detach().clone(), c.detach().clone(), feats.grad.clone(), pooled.grad.clone()]
    out += [p.grad.clone() for p in block.parameters() if p.grad is not None]
    out += [getattr(block, "bn%d" % i).running_var.clone() for i in range(1, 14)]
    return out


@pytest.mark.parametrize("mesh,batch", [("uv_sphere_482", 16), ("icosphere_162", 5)])
def test_one_launch_per_direction_equals_the_launch_per_layer(gpu, mesh, batch):
    """deform.chain: forward and backward of the block's thirteen hidden layers as ONE launch each against the thirteen launches
    (same bodies, the rows between layers travel through memory with agent-scope accesses behind per-vertex counters): every
    output, gradient and running statistic bit for bit, five times over (a race would not repeat)."""
    nv, adj, csr = _mesh(mesh, gpu)
    from geometrics_amd import _lib
    assert _lib.lib().geom_deform_chain_fits(nv) == 1
    torch.manual_seed(16)
    block = models.BatchMeshDeformationBlock(3 + 197, nv).to(gpu).train()
    feats = torch.randn(batch, nv, 3, device=gpu, requires_grad=True)
    pooled = torch.randn(batch, nv, 197, device=gpu, requires_grad=True)
    try:
        deform.chain = False
        ref = _block_step(block, feats, pooled, adj)
        deform.chain = True
        for _ in range(5):
            got = _block_step(block, feats, pooled, adj)
            assert len(got) == len(ref)
            for a, b in zip(got, ref):
                assert torch.equal(a, b)
    finally:
        deform.chain = True


def test_chain_launches_belong_to_one_stream_and_need_a_resident_grid(gpu):
    nv, adj, csr = _mesh("uv_sphere_482", gpu)
    from geometrics_amd import _lib
    lib = _lib.lib()
    assert lib.geom_deform_chain_fits(482) == 1 and lib.geom_deform_chain_fits(100000) == 0 and lib.geom_deform_chain_fits(0) == 0
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(a):
        assert deform.chain_fits(nv, gpu)                    # (everything idle: the launches move to stream a)
        busy = torch.empty(1 << 28, device=gpu)
        for _ in range(20):
            busy.fill_(1.0)                                   # stream a has work in flight ...
        with torch.cuda.stream(b):
            assert not deform.chain_fits(nv, gpu)            # ... so stream b issues its layers one by one
        assert deform.chain_fits(nv, gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(b):
        assert deform.chain_fits(nv, gpu)                    # the owner is idle: the launches move
    # a mesh with more vertices than workgroups fit the chip: the block runs on the layer-by-layer launches, same results as ever
    V, Fc = meshgen.icosphere(3)                              # 642 vertices
    assert lib.geom_deform_chain_fits(V.shape[0]) == 0
    adj642 = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    torch.manual_seed(17)
    block = models.BatchMeshDeformationBlock(3 + 197, V.shape[0]).to(gpu).train()
    feats = torch.randn(4, V.shape[0], 3, device=gpu, requires_grad=True)
    pooled = torch.randn(4, V.shape[0], 197, device=gpu, requires_grad=True)
    got = _block_step(block, feats, pooled, adj642)
    try:
        deform.enabled = False
        ref = _block_step(block, feats, pooled, adj642)
    finally:
        deform.enabled = True
    assert _maxrel(got[0], ref[0]) < 5e-5 and _maxrel(got[1], ref[1]) < 5e-5


def test_a_second_backward_over_a_retained_graph_takes_the_launches_per_layer(gpu):
    """The chain launch's counters are good for one pass (they count up from zero): backward(retain_graph=True) twice gives
    the gradients of one pass twice -- the second pass on the launches per layer, bit for bit the same."""
    nv, adj, csr = _mesh("uv_sphere_482", gpu)
    torch.manual_seed(18)
    block = models.BatchMeshDeformationBlock(3 + 197, nv).to(gpu).train()
    feats = torch.randn(16, nv, 3, device=gpu, requires_grad=True)
    pooled = torch.randn(16, nv, 197, device=gpu, requires_grad=True)
    f, c = block(feats, pooled, adj)
    loss = (f * f).sum() + c.sum()
    loss.backward(retain_graph=True)
    once = [p.grad.clone() for p in block.parameters() if p.grad is not None] + [pooled.grad.clone()]
    for p in block.parameters():
        p.grad = None
    pooled.grad = feats.grad = None
    loss.backward()
    again = [p.grad for p in block.parameters() if p.grad is not None] + [pooled.grad]
    for a, b in zip(once, again):
        assert torch.equal(a, b)


def test_chain_launches_under_a_busy_neighbour_stream(gpu):
    """The chain launches while another stream keeps the chip busy with ordinary kernels (their workgroups come and go, so the
    chain's are not all resident from the first cycle: late workgroups are waited for, never deadlocked on), forty steps:
    every step's outputs and gradients bit for bit those of the launches per layer."""
    nv, adj, csr = _mesh("uv_sphere_482", gpu)
    torch.manual_seed(19)
    block = models.BatchMeshDeformationBlock(3 + 197, nv).to(gpu).train()
    feats = torch.randn(16, nv, 3, device=gpu, requires_grad=True)
    pooled = torch.randn(16, nv, 197, device=gpu, requires_grad=True)
    try:
        deform.chain = False
        ref = _block_step(block, feats, pooled, adj)
    finally:
        deform.chain = True
    torch.cuda.synchronize()
    noise = torch.cuda.Stream()
    junk = torch.empty(1 << 26, device=gpu)
    a, b = torch.randn(2048, 2048, device=gpu), torch.randn(2048, 2048, device=gpu)
    for step in range(40):
        with torch.cuda.stream(noise):
            for _ in range(6):
                junk.fill_(float(step))
                torch.mm(a, b)
        got = _block_step(block, feats, pooled, adj)
        for x, y in zip(got, ref):
            assert torch.equal(x, y), "step %d" % step
    torch.cuda.synchronize()


def _spy_chain(monkeypatch, forbid=False):
    """The names of the chain launches asked for from here on: deform.chain_forward / chain_backward still run, or with
    forbid = True fail the test instead of launching."""
    calls = []
    for name in ("chain_forward", "chain_backward"):
        real = getattr(deform, name)

        def spy(*a, _real=real, _name=name, **k):
            calls.append(_name)
            if forbid:
                raise AssertionError("%s asked for on a directed adjacency" % _name)
            return _real(*a, **k)
        monkeypatch.setattr(deform, name, spy)
    return calls


# case -> (deform.serves at the case's shape, chain launches taken)
_BLOCK192_ROUTES = {"train482": (True, True), "smooth482": (True, True), "ico162_bn": (True, True), "ico162_b24": (False, False)}


@pytest.mark.parametrize("case", BLOCK192_CASES)
def test_block192_against_the_reference_fixture(gpu, case, monkeypatch):
    """The block at the width that ships (192) against the REFERENCE's BatchMeshDeformationBlock(195, V) run in float64
    (tests/golden/block192.npz): train482 = the reference's training shape on the fused chain launches (482 vertices, two
    33-entry poles: table + tail); smooth482 = the same without the ReLUs (deform.relu = False; the reference's F.relu made the
    identity); ico162_bn = batch 5 (rows beyond the batch are zero rows of the tile) with per-layer BatchNorm settings that
    differ from bn1's; ico162_b24 = batch 24 on the separate operators and the library BatchNorm (24 x 192 > 4096 values per
    vertex).  After the step, where stored, the eval-mode forward under no_grad with the updated running statistics (the
    reference driver's validation loop).  Every stored gradient ELEMENT is held to 5e-5 of its tensor's scale, in the ReLU
    cases too: their fixture keeps every float64 pre-activation at least 2e-5 from the ReLU's kink (make_golden.py
    _off_the_kink), so no fp32 evaluation switches a unit (one switched unit of layer 6 moved the parameter gradients of
    layers 1-6 by up to 6e-3 of their scale)."""
    g = block192_fixture(case)
    inp = block192_case(g)                    # (checksums of the regenerated inputs asserted)
    b, nv = int(g["batch"]), int(g["nv"])
    relu = bool(g["relu"])
    V, Fc = meshgen.uv_sphere() if str(g["mesh"]) == "uv_sphere_482" else meshgen.icosphere(2)
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    a = adj.cpu().numpy()
    r, c = np.nonzero(a)
    assert np.array_equal(r, g["adj_rows"]) and np.array_equal(c, g["adj_cols"]) and np.array_equal(bits(a[r, c]), bits(g["adj_vals"]))
    csr = layers.adjacency_csr(adj)
    block = block192_parameters(models.BatchMeshDeformationBlock(195, nv), g).to(gpu).train()     # (checksums asserted)
    named = dict(block.named_parameters())
    to = lambda k: torch.from_numpy(inp[k]).to(gpu)          # noqa: E731
    feats, pooled = to("features").requires_grad_(True), to("pooled").requires_grad_(True)
    serves, chained = _BLOCK192_ROUTES[case]
    assert deform.serves(block, feats, pooled, csr) == serves
    if not serves:
        assert not block.bn1.fused_kernel_serves(torch.empty(b, nv, 192, device=gpu))      # the library BatchNorm
    calls = _spy_chain(monkeypatch)
    monkeypatch.setattr(deform, "relu", relu)
    out_f, coords = block(feats, pooled, adj)
    ((out_f * to("g_features")).sum() + (coords * to("g_coords")).sum()).backward()
    assert calls == (["chain_forward", "chain_backward"] if chained else [])
    monkeypatch.setattr(deform, "relu", True)
    sd = block.state_dict()
    assert all(int(sd["bn%d.num_batches_tracked" % i]) == 1 for i in range(1, 14)) and int(sd["bn14.num_batches_tracked"]) == 0
    assert all(named[k].grad is None for k in named if k.startswith("bn14"))
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
    assert set(stored) == {k for k in g if k in stored}

    def maxrel(x, y):
        return float(np.abs(x - y).max()) / max(float(np.abs(y).max()), 1e-30)

    def tensors(key, x):          # (the 13 layers' stacked vectors are 13 tensors)
        if key in ("grad.gc_bias", "grad.bn_weight", "grad.bn_bias", "running_mean", "running_var"):
            return [("%s %s[layer %d]" % (case, key, i + 1), t) for i, t in enumerate(x)]
        return [("%s %s" % (case, key), x)]
    bad = []
    for key, got in stored.items():
        for (what, x), (_, y) in zip(tensors(key, got), tensors(key, g[key].astype(np.float64))):
            if not key.startswith("grad."):          # forward, eval forward, running statistics
                bar = 1e-5 if key.startswith("running") else 2e-5
                if not log_margin(what + " max-norm", maxrel(x, y), bar):
                    bad.append("%s: %.2e of scale (bar %g)" % (what, maxrel(x, y), bar))
            elif not log_margin(what + " max-norm", maxrel(x, y), 5e-5):     # every gradient element
                bad.append("%s: %.2e of scale (bar 5e-5)" % (what, maxrel(x, y)))
    for name, (want, scale) in zip(g["ck_names"], g["ck"]):
        name = str(name)
        bar = 1e-5 if name.startswith("running") else 2e-5 if not name.startswith("grad.") else 5e-5
        err = abs(weighted_checksum(name, full[name])[0] - want) / scale
        if not log_margin("%s checksum %s" % (case, name), err, bar):
            bad.append("checksum of %s: %.2e of its scale (bar %g)" % (name, err, bar))
    assert not bad, "; ".join(bad)


def _directed_482():
    """The 482-vertex template's normalised adjacency made DIRECTED (host tensor): A[u][v] deleted for every third edge
    u < v (A[v][u] kept), and one-way entries between vertices far apart in the numbering -- different XCD runs of the
    launches' vertex order (db_vertex: runs of 61 vertices).  Rows stay within the 8-wide table + the tail."""
    V, Fc = meshgen.uv_sphere()
    a = utils.adj_init(torch.from_numpy(Fc))["adj"].clone()
    u, v = np.nonzero(np.triu(a.numpy(), 1))
    a[u[::3], v[::3]] = 0.0
    for p, q in ((10, 400), (100, 300), (200, 470), (300, 30), (450, 60), (130, 250)):
        assert a[p, q] == 0 and a[q, p] == 0
        a[p, q] = 0.125
    return a


@pytest.mark.parametrize("relu", [False, True])
def test_block_on_a_directed_adjacency(gpu, relu, monkeypatch):
    """A directed adjacency (A[u][v] != 0 where A[v][u] == 0) may not take the chain launch: there vertex v rewrites its support
    row once the vertices of ITS row are past the previous layer, and u, which gathers v's row, is not among them.  The block
    takes the fused launches per layer instead (and, deform.enabled = False, the separate operators): both against the
    float64 restatement on the same dense adjacency, at the bars of test_the_fused_block_against_float64... (relu=False:
    deform.relu applies to the fused launches only, so the separate operators are compared under ReLU).  A symmetric
    pattern with asymmetric values -- the row-normalised mesh adjacency itself -- still takes the chain."""
    import copy
    adj = _directed_482().to(gpu)
    nv = adj.shape[0]
    csr = layers.adjacency_csr(adj)
    assert not csr.symmetric_structure and csr.ell_w == 8 and csr.over is not None
    assert not torch.equal(adj != 0, (adj != 0).t())
    torch.manual_seed(20)
    block = models.BatchMeshDeformationBlock(3 + 200, nv).to(gpu).train()
    with torch.no_grad():
        for i in range(1, 14):
            getattr(block, "bn%d" % i).weight.uniform_(0.5, 1.5)
            getattr(block, "bn%d" % i).bias.uniform_(-0.3, 0.3)
    feats = torch.randn(16, nv, 3, device=gpu)
    pooled = torch.randn(16, nv, 200, device=gpu)
    g_f, g_c = torch.randn(16, nv, 192, device=gpu), torch.randn(16, nv, 3, device=gpu)
    f64, p64 = feats.double().cpu().requires_grad_(True), pooled.double().cpu().requires_grad_(True)
    e_f, e_c, params64 = _block64(block, f64, p64, adj, relu)
    ((e_f * g_f.double().cpu()).sum() + (e_c * g_c.double().cpu()).sum()).backward()
    calls = _spy_chain(monkeypatch, forbid=True)
    for fused in ((True, False) if relu else (True,)):
        blk = copy.deepcopy(block)
        monkeypatch.setattr(deform, "enabled", fused)
        monkeypatch.setattr(deform, "relu", relu)
        f, p = feats.clone().requires_grad_(True), pooled.clone().requires_grad_(True)
        assert deform.serves(blk, f, p, csr) == fused
        out_f, coords = blk(f, p, adj)
        ((out_f * g_f).sum() + (coords * g_c).sum()).backward()
        assert calls == []
        assert _maxrel(out_f, e_f) <= 2e-5 and _maxrel(coords, e_c) <= 2e-5
        named = dict(blk.named_parameters())
        pairs = [(n, q.grad, params64[n].grad) for n, q in named.items() if not n.startswith("bn14")]
        pairs += [("features", f.grad, f64.grad), ("pooled", p.grad, p64.grad)]
        for name, got, want in pairs:
            if relu:
                assert _l2rel(got, want) <= 5e-3, "%s (fused %s): %.2e from float64 in the L2 norm" % (name, fused, _l2rel(got, want))
            else:
                assert _maxrel(got, want) <= 5e-5, "%s: %.2e of scale from float64" % (name, _maxrel(got, want))
    monkeypatch.undo()              # (deform.enabled / relu back to True, the launches unwrapped)
    calls = _spy_chain(monkeypatch)
    nv, sym, csr = _mesh("uv_sphere_482", gpu)
    assert csr.symmetric_structure and not torch.equal(sym, sym.t())
    out_f, coords = block(feats.clone().requires_grad_(True), pooled, sym)
    (out_f.sum() + coords.sum()).backward()
    assert calls == ["chain_forward", "chain_backward"]


def test_a_block_for_another_vertex_count_raises_before_any_launch(gpu):
    """A block built for 162 vertices given 482-vertex inputs raises as the reference's nn.BatchNorm1d does, on the fused
    route and on the separate operators, before any BatchNorm launch (which would index the 162-entry parameters and
    statistics by vertices up to 481): the launches never serve the call, and VertexBatchNorm checks on the host."""
    nv, adj, csr = _mesh("uv_sphere_482", gpu)
    block = models.BatchMeshDeformationBlock(3 + 197, 162).to(gpu).train()
    f, p = torch.randn(16, nv, 3, device=gpu), torch.randn(16, nv, 197, device=gpu)
    assert not deform.serves(block, f, p, csr)
    try:
        for fused in (True, False):
            deform.enabled = fused
            with pytest.raises(RuntimeError, match="running_mean should contain 482 elements not 162"):
                block(f, p, adj)
    finally:
        deform.enabled = True
    torch.cuda.synchronize()
    assert all(bool((getattr(block, "bn%d" % i).running_mean == 0).all()) for i in range(1, 15))
