"""-m gpu: the eval-mode forward of the 192-wide mesh deformation block (geom_deform_infer_fwd_f32, deform.inference_chain;
reference models.py:237-297 under eval() and no_grad, as GEOMetrics.py's validate / evaluate run it):

* one launch against the separate operators it replaces -- aggregation + per-vertex BatchNorm (running statistics) + ReLU +
  residual average bit for bit, the next layer's product within the fp32 summation bound;
* the block against the reference run in float64 (tests/golden/block192_eval.npz) and against the separate operators;
* the route: thirteen inference launches per eval forward under no_grad, none with gradients enabled, nothing written to the
  BatchNorm state, the training step's chain launches unchanged afterwards;
* the eval forward captured in a HIP graph; a directed adjacency; the driver's input forms (stride-0 expand, torch.cat)."""

import numpy as np
import pytest
import torch

from geometrics_amd import _lib, deform, layers, meshgen, models, utils
from deform_eval_helpers import EVAL_CASES, eval_block, eval_fixture
from helpers import block64, fill_block_parameters, weighted_checksum

pytestmark = pytest.mark.gpu


def _mesh(name, gpu):
    V, Fc = meshgen.uv_sphere() if name == "uv_sphere_482" else meshgen.icosphere(2)
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    return V.shape[0], adj, layers.adjacency_csr(adj)


def _maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _spy_calls(monkeypatch):
    """Names of every library entry point called from here on (_lib.call), and of deform's chain launches."""
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    for name in ("chain_forward", "chain_backward"):
        fn = getattr(deform, name)

        def chain_spy(*a, _fn=fn, _name=name, **k):
            calls.append(_name)
            return _fn(*a, **k)
        monkeypatch.setattr(deform, name, chain_spy)
    return calls


def _layer_inputs(gpu, nv, batch, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    c = 192

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(gpu)
    s, res = rnd(batch, nv, c), rnd(batch, nv, c)
    bias = rnd(c, scale=0.1)
    gamma, beta = (torch.rand(nv, generator=g) + 0.5).to(gpu), rnd(nv, scale=0.2)
    # running statistics over the ranges the reference's pretrained checkpoints hold: variances log-uniform in [0.05, 400],
    # means in +-5
    rv = torch.exp(torch.empty(nv).uniform_(np.log(0.05), np.log(400.0), generator=g)).to(gpu)
    rm = torch.empty(nv).uniform_(-5.0, 5.0, generator=g).to(gpu)
    w = rnd(c, c, scale=1 / 14)
    return s, res, bias, gamma, beta, rm, rv, w


def _product_within_bound(s_next, x, w):
    """s_next = x . w within the elementwise bound of an fp32 sum of 192 products (test_deform_gpu.py:65-67)."""
    c = w.shape[0]
    x64, w64 = x.double().cpu(), w.double().cpu()
    s64 = x64 @ w64
    bound = (c + 8) * 2.0 ** -24 * (x64.abs() @ w64.abs())
    return bool(((s_next.double().cpu() - s64).abs() <= bound + 1e-30).all())


@pytest.mark.parametrize("residual", [False, True])
# (batch 18 x 482 rows = 543 row-blocks on 512 workgroups: some take a second row-block, behind the slice they hold already)
@pytest.mark.parametrize("mesh,batch", [("uv_sphere_482", 1), ("uv_sphere_482", 16), ("icosphere_162", 5), ("uv_sphere_482", 18)])
def test_one_inference_launch_against_the_separate_operators(gpu, mesh, batch, residual, monkeypatch):
    nv, adj, csr = _mesh(mesh, gpu)
    s, res, bias, gamma, beta, rm, rv, w = _layer_inputs(gpu, nv, batch, 31 + batch)
    res = res if residual else None
    eps = 1e-5
    x, s_next = torch.empty_like(s), torch.empty_like(s)
    packed, _ = deform.pack_weights([w])
    rm0, rv0 = rm.clone(), rv.clone()
    deform.infer_layer_forward(s, bias, csr, gamma, beta, rm, rv, eps, True, res, 0.5, x, w_next=packed[0], s_out=s_next)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)           # the running statistics are read, never written
    # the separate operators: the aggregation, then geom_vertex_bn_fwd_f32's eval branch (+ ReLU + residual average)
    bn = models.VertexBatchNorm(nv).to(gpu).eval()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
        bn.eps = eps
        calls = _spy_calls(monkeypatch)
        z_ref = layers.zero_n_aggregate(s, adj, bias, 64, None)
        x_ref = bn(z_ref, relu=True, residual=res, scale=0.5)
    assert "geom_vertex_bn_fwd_f32" in calls
    monkeypatch.undo()
    assert torch.equal(x.view(torch.int32), x_ref.view(torch.int32)), "X' differs from the separate operators' bits"
    assert _product_within_bound(s_next, x, w)
    # the last layer: no product, the final features and the coordinate head's raw support
    w_head = (torch.randn(192, 3, device=gpu) / 14).contiguous()
    x2, s_head = torch.empty_like(s), torch.empty(batch, nv, 3, device=gpu)
    deform.infer_layer_forward(s, bias, csr, gamma, beta, rm, rv, eps, True, res, 0.5, x2, w_head=w_head, s_head=s_head)
    assert torch.equal(x2.view(torch.int32), x_ref.view(torch.int32))
    assert _product_within_bound(s_head, x2, w_head)
    # X' needed by nobody (an odd layer): only the product is written
    s_only = torch.full_like(s, float("nan"))
    deform.infer_layer_forward(s, bias, csr, gamma, beta, rm, rv, eps, True, res, 0.5, None, w_next=packed[0], s_out=s_only)
    assert torch.equal(s_only, s_next)


def test_one_inference_launch_at_batch_40_against_float64(gpu):
    """B = 40 (1 205 row-blocks: workgroups take several in turn): the separate BatchNorm is the library's there (b * c >
    4096), so X' is held against float64 at 2e-6 of scale."""
    nv, adj, csr = _mesh("uv_sphere_482", gpu)
    s, res, bias, gamma, beta, rm, rv, w = _layer_inputs(gpu, nv, 40, 40)
    eps = 1e-5
    x, s_next = torch.empty_like(s), torch.empty_like(s)
    packed, _ = deform.pack_weights([w])
    deform.infer_layer_forward(s, bias, csr, gamma, beta, rm, rv, eps, True, res, 0.5, x, w_next=packed[0], s_out=s_next)
    s64, a64 = s.double().cpu(), adj.double().cpu()
    z64 = torch.cat((a64 @ s64[..., :64], s64[..., 64:]), dim=-1) + bias.double().cpu()
    m, v = rm.double().cpu().view(1, -1, 1), rv.double().cpu().view(1, -1, 1)
    y64 = (z64 - m) / (v + eps).sqrt() * gamma.double().cpu().view(1, -1, 1) + beta.double().cpu().view(1, -1, 1)
    x64 = (res.double().cpu() + torch.relu(y64)) * 0.5
    assert _maxrel(x, x64) <= 2e-6
    assert _product_within_bound(s_next, x, w)


def _to(g, gpu):
    return (torch.from_numpy(g["features"]).to(gpu), torch.from_numpy(g["pooled"]).to(gpu),
            torch.from_numpy(g["adj"]).to(gpu))


@pytest.mark.parametrize("case", EVAL_CASES)
def test_block_against_the_eval_fixture(gpu, case, monkeypatch):
    g = eval_fixture(case)
    block = eval_block(g, gpu)
    feats, pooled, adj = _to(g, gpu)
    calls = _spy_calls(monkeypatch)
    with torch.no_grad():
        assert deform.serves_inference(block, feats, pooled, layers.adjacency_csr(adj))
        out_f, coords = block(feats, pooled, adj)
    monkeypatch.undo()
    f, c = out_f.double().cpu().numpy(), coords.double().cpu().numpy()
    rb, rv, m = (g[k].astype(np.int64) for k in ("rows_b", "rows_v", "meshes"))
    for name, got, want in (("features_rows", f[rb, rv], g["features_rows"]), ("coords", c[m], g["coords"])):
        want = want.astype(np.float64)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print("%s %s: %.2e of scale (bar 2e-5)" % (case, name, err))
        assert err <= 2e-5, "%s: %.2e of scale" % (name, err)
    full = {"features": f, "coords": c}
    for name, (want, scale) in zip(g["ck_names"], g["ck"]):
        got = weighted_checksum(str(name), full[str(name)])[0]
        print("%s checksum %s: %.2e of scale (bar 2e-5)" % (case, name, abs(got - want) / scale))
        assert abs(got - want) <= 2e-5 * scale
    # the same block on the separate operators
    monkeypatch.setattr(deform, "enabled", False)
    with torch.no_grad():
        ref_f, ref_c = block(feats, pooled, adj)
    print("%s against the separate operators: features %.2e, coords %.2e" % (case, _maxrel(out_f, ref_f), _maxrel(coords, ref_c)))
    assert _maxrel(out_f, ref_f) <= 2e-5 and _maxrel(coords, ref_c) <= 2e-5
    assert calls.count("geom_deform_infer_fwd_f32") == 13


def _block482(gpu, seed):
    nv, adj, csr = _mesh("uv_sphere_482", gpu)
    block = fill_block_parameters(models.BatchMeshDeformationBlock(195, nv), seed).to(gpu)
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for i in range(1, 14):
            bn = getattr(block, "bn%d" % i)
            bn.running_var.copy_(torch.exp(torch.empty(nv).uniform_(np.log(0.05), np.log(400.0), generator=g)))
            bn.running_mean.copy_(torch.empty(nv).uniform_(-5.0, 5.0, generator=g))
    return nv, adj, csr, block


@pytest.mark.parametrize("batch", [1, 16, 40])
def test_an_eval_forward_takes_the_inference_launches(gpu, batch, monkeypatch):
    nv, adj, csr, block = _block482(gpu, 50 + batch)
    block.eval()
    feats, pooled = torch.randn(batch, nv, 3, device=gpu), torch.randn(batch, nv, 192, device=gpu)
    calls = _spy_calls(monkeypatch)
    # (every batch is served: the launches beat the separate operators at 1, 16 and 40, profiles/eval_forward.txt)
    with torch.no_grad():
        assert deform.serves_inference(block, feats, pooled, csr)
        block(feats, pooled, adj)
    assert calls.count("geom_deform_infer_fwd_f32") == 13
    assert calls.count("geom_deform_pack_weights_zero_f32") == 1
    assert "geom_vertex_bn_fwd_f32" not in calls and "chain_forward" not in calls
    # eval with gradients enabled (frozen-BatchNorm fine-tuning): no inference launch, today's route
    del calls[:]
    out = block(feats, pooled, adj)
    assert out[0].requires_grad
    with_grad = list(calls)
    assert "geom_deform_infer_fwd_f32" not in with_grad and "chain_forward" not in with_grad
    del calls[:]
    monkeypatch.setattr(deform, "enabled", False)
    block(feats, pooled, adj)
    assert calls == with_grad


def test_an_eval_forward_leaves_the_state_and_the_training_route_alone(gpu, monkeypatch):
    nv, adj, csr, block = _block482(gpu, 60)
    feats, pooled = torch.randn(16, nv, 3, device=gpu), torch.randn(16, nv, 192, device=gpu)
    before = {k: v.clone() for k, v in block.state_dict().items()}
    block.eval()
    with torch.no_grad():
        assert deform.serves_inference(block, feats, pooled, csr)
        block(feats, pooled, adj)
    after = block.state_dict()
    assert sorted(after) == sorted(before)
    for k, v in after.items():           # bit for bit (the floating-point tensors compared as their bit patterns)
        if v.is_floating_point():
            assert torch.equal(v.view(torch.int32), before[k].view(torch.int32)), k
        else:
            assert torch.equal(v, before[k]), k
    # a training step afterwards still takes the one-launch chains
    block.train()
    calls = _spy_calls(monkeypatch)
    f, p = feats.clone().requires_grad_(True), pooled.clone().requires_grad_(True)
    out_f, coords = block(f, p, adj)
    (out_f.sum() + coords.sum()).backward()
    assert calls.count("chain_forward") == 1 and calls.count("chain_backward") == 1
    assert "geom_deform_infer_fwd_f32" not in calls
    assert int(block.state_dict()["bn1.num_batches_tracked"]) == int(before["bn1.num_batches_tracked"]) + 1


@pytest.mark.parametrize("batch", [1, 16])
def test_the_eval_forward_replays_inside_a_hip_graph(gpu, batch):
    nv, adj, csr, block = _block482(gpu, 70 + batch)
    block.eval()
    feats, pooled = torch.randn(batch, nv, 3, device=gpu), torch.randn(batch, nv, 192, device=gpu)
    with torch.no_grad():
        assert deform.serves_inference(block, feats, pooled, csr)
        eager_f, eager_c = (t.clone() for t in block(feats, pooled, adj))      # (the eager call: the adjacency's tables)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph):
                static_f, static_c = block(feats, pooled, adj)
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_f.view(torch.int32), eager_f.view(torch.int32))
        assert torch.equal(static_c.view(torch.int32), eager_c.view(torch.int32))
        # new inputs into the static buffers
        feats.copy_(torch.randn_like(feats)), pooled.copy_(torch.randn_like(pooled))
        want_f, want_c = (t.clone() for t in block(feats, pooled, adj))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_f.view(torch.int32), want_f.view(torch.int32))
        assert torch.equal(static_c.view(torch.int32), want_c.view(torch.int32))
        assert not torch.equal(want_f, eager_f)


def _directed_482():
    """The 482-vertex template's normalised adjacency made DIRECTED (host tensor), as test_deform_gpu.py builds it: A[u][v]
    deleted for every third edge u < v (A[v][u] kept), and one-way entries between vertices far apart in the numbering."""
    V, Fc = meshgen.uv_sphere()
    a = utils.adj_init(torch.from_numpy(Fc))["adj"].clone()
    u, v = np.nonzero(np.triu(a.numpy(), 1))
    a[u[::3], v[::3]] = 0.0
    for p, q in ((10, 400), (100, 300), (200, 470), (300, 30), (450, 60), (130, 250)):
        assert a[p, q] == 0 and a[q, p] == 0
        a[p, q] = 0.125
    return a


def test_the_eval_forward_on_a_directed_adjacency(gpu, monkeypatch):
    adj = _directed_482().to(gpu)
    nv = adj.shape[0]
    csr = layers.adjacency_csr(adj)
    assert not csr.symmetric_structure and csr.ell_w == 8 and csr.over is not None
    _, _, _, block = _block482(gpu, 80)
    block.eval()
    feats, pooled = torch.randn(4, nv, 3, device=gpu), torch.randn(4, nv, 192, device=gpu)
    calls = _spy_calls(monkeypatch)
    with torch.no_grad():
        assert deform.serves_inference(block, feats, pooled, csr)
        out_f, coords = block(feats, pooled, adj)
    assert calls.count("geom_deform_infer_fwd_f32") == 13
    running = {i: (getattr(block, "bn%d" % i).running_mean.double().cpu(), getattr(block, "bn%d" % i).running_var.double().cpu())
               for i in range(1, 14)}
    with torch.no_grad():
        e_f, e_c, _ = block64(block, feats.double().cpu(), pooled.double().cpu(), adj, relu=True, running=running)
    assert _maxrel(out_f, e_f) <= 2e-5 and _maxrel(coords, e_c) <= 2e-5


def test_the_drivers_input_forms(gpu, monkeypatch):
    """GEOMetrics.py:205-218 hands the block a stride-0 `expand` of the template positions and a `torch.cat` result: served by
    the inference launches, equal to the separate operators at the block bar."""
    _, adj, csr, block = _block482(gpu, 90)
    block.eval()
    V, _ = meshgen.uv_sphere()
    nv = V.shape[0]
    positions = torch.from_numpy(V).to(gpu).unsqueeze(0).expand(2, nv, 3)
    assert positions.stride(0) == 0
    pooled = torch.cat((torch.randn(2, nv, 100, device=gpu), torch.randn(2, nv, 92, device=gpu)), dim=-1)
    calls = _spy_calls(monkeypatch)
    with torch.no_grad():
        out_f, coords = block(positions, pooled, adj)
    assert calls.count("geom_deform_infer_fwd_f32") == 13
    monkeypatch.setattr(deform, "enabled", False)
    with torch.no_grad():
        ref_f, ref_c = block(positions, pooled, adj)
    assert _maxrel(out_f, ref_f) <= 2e-5 and _maxrel(coords, ref_c) <= 2e-5


def test_a_wide_residual_beyond_the_32_bit_offsets(gpu, monkeypatch):
    """Layer 2's residual is the block input's leading 192 columns, read in place at the input's pitch (1155 for the driver's
    second and third blocks).  At b * nv * 1155 >= 2^29 -- here 2 870 meshes of 162 vertices, inside serves_inference's
    b * nv * 192 < 2^29 -- its byte offsets would pass 32 bits: the launch wrapper copies it to pitch 192.  One launch with it
    equals the launch with a contiguous residual bit for bit, and the block is served and agrees with the separate operators
    on a few of its meshes."""
    nv, adj, csr = _mesh("icosphere_162", gpu)
    batch = 2870
    assert batch * nv * 1155 >= 2 ** 29 and batch * nv * 192 < 2 ** 29
    g = torch.Generator(device="cpu").manual_seed(95)
    s = torch.randn(batch, nv, 192, generator=g).to(gpu)
    wide = torch.randn(batch, nv, 1155, generator=g).to(gpu)
    lead = wide[..., :192]
    _, _, bias, gamma, beta, rm, rv, w = _layer_inputs(gpu, nv, 1, 96)
    packed, _ = deform.pack_weights([w])
    x_wide, x_contig = torch.empty_like(s), torch.empty_like(s)
    deform.infer_layer_forward(s, bias, csr, gamma, beta, rm, rv, 1e-5, True, lead, 0.5, x_wide, w_head=w[:, :3].contiguous(),
                               s_head=torch.empty(batch, nv, 3, device=gpu))
    deform.infer_layer_forward(s, bias, csr, gamma, beta, rm, rv, 1e-5, True, lead.contiguous(), 0.5, x_contig,
                               w_head=w[:, :3].contiguous(), s_head=torch.empty(batch, nv, 3, device=gpu))
    assert torch.equal(x_wide.view(torch.int32), x_contig.view(torch.int32))
    del s, x_wide, x_contig, lead
    # the block: features [B,V,3] + pooled [B,V,1152] -> a 1155-wide input
    block = fill_block_parameters(models.BatchMeshDeformationBlock(1155, nv), 97).to(gpu).eval()
    feats, pooled = wide[..., :3].contiguous(), wide[..., 3:].contiguous()
    del wide
    calls = _spy_calls(monkeypatch)
    with torch.no_grad():
        assert deform.serves_inference(block, feats, pooled, csr)
        out_f, coords = block(feats, pooled, adj)
    assert calls.count("geom_deform_infer_fwd_f32") == 13
    pick = torch.tensor([0, 1, batch - 1], device=gpu)
    monkeypatch.setattr(deform, "enabled", False)
    with torch.no_grad():
        ref_f, ref_c = block(feats[pick], pooled[pick], adj)
    assert _maxrel(out_f[pick], ref_f) <= 2e-5 and _maxrel(coords[pick], ref_c) <= 2e-5
