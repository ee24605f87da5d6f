"""-m gpu: which entry points the 0N-GCN aggregation act([A . S[..., :k] | S[..., k:]] + bias) issues, and that every route
computes what the generic CSR kernel computes (geometrics_amd/aggregation.py, csrc/zn_gcn.hip).

* the route pin: the library entry points of one warmed-up forward + backward, `call` / `check` prefix and order included,
  against the lists below, worked out from the separate operators' host code (`GEOM_ROUTE_LOG=file` writes what a run issues,
  to record them; the recorder is tests/test_products_gpu.py's);
* the values: every table route sums a row's neighbours in CSR order, so output and input gradient carry the SAME BITS as
  `geom_zn_gcn_aggregate_{fwd,bwd}_f32` called directly; the bias gradient (another partial layout per route) against
  float64 with the bound of tests/test_aggregate_any_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden
from geometrics_amd import _lib as L
from geometrics_amd import fused, layers, meshgen, utils
from test_products_gpu import issued

pytestmark = pytest.mark.gpu

B = 2
_CODES = {None: 0, F.relu: 1, F.elu: 2}      # any other callable: applied outside an un-activated kernel


@pytest.fixture(scope="module")
def meshes(gpu):
    """name -> what a layer takes as `adj`: the 162-vertex icosphere (table width 8, no tail), the 482-vertex template (two
    33-entry poles in the CSR tail) and a dense random graph whose rows are too long for a table."""
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    sphere = layers.adjacency_csr(utils.adj_init(to(meshgen.icosphere(2)[1]))["adj"])
    template = layers.adjacency_csr(utils.adj_init(to(golden("adj_482")["faces"]))["adj"])
    g = torch.Generator(device="cpu").manual_seed(48)
    dense = (torch.rand(48, 48, generator=g) < 0.5).float()
    dense.fill_diagonal_(1.0)
    dense = dense.to(gpu)
    assert sphere.nv == 162 and sphere.ell_w == 8 and sphere.over is None and sphere.over_t is None
    assert template.nv == 482 and template.ell_w == 8 and template.over is not None
    assert layers.adjacency_csr(dense).ell_w == 0
    return {"sphere": sphere, "template": template, "dense": dense}


def _entry_points(step, monkeypatch):
    """The library entry points the second call of step() issues (the recorder's other lines, the product wrappers and
    torch's products with their shapes, are tests/test_products_gpu.py's subject)."""
    return [event for event in issued(step, monkeypatch) if event.startswith(("call ", "check "))]


def _log(name, events):
    log = os.environ.get("GEOM_ROUTE_LOG")
    if log:
        with open(log, "a") as f:
            f.write("%s\n    %s\n" % (name, "\n    ".join(events)))


def _expected(name):
    return [line.strip() for line in ROUTES[name].strip().split("\n") if line.strip()]


def _csr_kernel(csr, sup, bias, k, activation, seed):
    """The generic CSR kernel called directly on [b, nv, c] operands: (output, input gradient, bias gradient in float64 and
    the mass its bound scales with).  A foreign activation is applied by torch on both sides of the comparison."""
    b, nv, c = sup.shape
    act = _CODES.get(activation, 0)
    pre = torch.empty_like(sup)
    L.call("geom_zn_gcn_aggregate_fwd_f32", b, nv, c, k, csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(),
           sup.data_ptr(), L.ptr(bias), act, pre.data_ptr())
    out, g = pre, seed
    if activation is not None and act == 0:
        leaf = pre.clone().requires_grad_(True)
        out = activation(leaf)
        out.backward(seed)
        out, g = out.detach(), leaf.grad.contiguous()
    scratch = torch.empty(L.lib().geom_zn_gcn_bwd_scratch_floats(b, nv, c), device=sup.device)
    grad_sup, grad_bias = torch.empty_like(sup), torch.empty(c, device=sup.device)
    L.call("geom_zn_gcn_aggregate_bwd_f32", b, nv, c, k, csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(), csr.val_t.data_ptr(),
           g.data_ptr(), pre.data_ptr(), act, grad_sup.data_ptr(), grad_bias.data_ptr(), scratch.data_ptr())
    gp = g.double()
    if act == 1:
        gp = gp * (pre > 0)
    elif act == 2:
        gp = torch.where(pre > 0, gp, gp * (pre.double() + 1))
    return out, grad_sup, gp.view(-1, c).sum(0), gp.abs().view(-1, c).sum(0)


def _bias_close(got, ref, mass):
    assert bool(((got.double() - ref).abs() <= 1e-6 * mass + 1e-30).all())


# name, mesh, support shape, k, activation, with bias
PLAIN = [("relu-192", "sphere", (B, 162, 192), 64, F.relu, True),
         ("elu-192", "sphere", (B, 162, 192), 64, F.elu, True),
         ("none-192", "sphere", (B, 162, 192), 64, None, True),
         ("tanh-192", "sphere", (B, 162, 192), 64, torch.tanh, True),
         ("any-width-300", "sphere", (B, 162, 300), 30, F.relu, True),
         ("split10-40", "sphere", (B, 162, 40), 4, F.relu, True),
         ("unbatched-192", "sphere", (162, 192), 64, F.relu, True),
         ("no-bias-192", "sphere", (B, 162, 192), 64, F.relu, False),
         ("template-192", "template", (B, 482, 192), 64, F.relu, True),
         ("no-table-192", "dense", (B, 48, 192), 64, F.relu, True),
         ("no-table-7", "dense", (B, 48, 7), 3, F.relu, True)]


def _operands(shape, gpu, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    sup = torch.randn(*shape, generator=g).to(gpu).requires_grad_(True)
    bias = torch.randn(shape[-1], generator=g).to(gpu).requires_grad_(True)
    return g, sup, bias


@pytest.mark.parametrize("case", PLAIN, ids=[case[0] for case in PLAIN])
def test_zero_n_aggregate_issues_what_it_issued_and_equals_the_csr_kernel(gpu, meshes, monkeypatch, case):
    name, mesh, shape, k, activation, with_bias = case
    adj = meshes[mesh]
    g, sup, bias = _operands(shape, gpu, 11 + len(name))
    seed = torch.randn(*shape, generator=g).to(gpu)
    if not with_bias:
        bias = None
    kept = {}

    def step():
        sup.grad = None
        if bias is not None:
            bias.grad = None
        kept["out"] = layers.zero_n_aggregate(sup, adj, bias, k, activation)
        kept["out"].backward(seed)
        torch.cuda.synchronize()
    events = _entry_points(step, monkeypatch)
    _log(name, events)
    three = (lambda t: t.detach().reshape((-1,) + shape[-2:]).contiguous())
    want_out, want_grad, ref, mass = _csr_kernel(layers.adjacency_csr(adj), three(sup), None if bias is None else bias.detach(),
                                                 k, activation, three(seed))
    assert torch.equal(three(kept["out"]), want_out)
    assert torch.equal(three(sup.grad), want_grad)
    if bias is not None:
        _bias_close(bias.grad, ref, mass)
    assert events == _expected(name)


def test_a_per_mesh_adjacency_issues_no_entry_point(gpu, meshes, monkeypatch):
    g, sup, bias = _operands((B, 48, 192), gpu, 5)
    adj = torch.stack([meshes["dense"], meshes["dense"].t().contiguous()])
    seed = torch.randn(B, 48, 192, generator=g).to(gpu)
    kept = {}

    def step():
        sup.grad = bias.grad = None
        kept["out"] = layers.zero_n_aggregate(sup, adj, bias, 64, F.relu)
        kept["out"].backward(seed)
        torch.cuda.synchronize()
    events = _entry_points(step, monkeypatch)
    _log("per-mesh", events)
    want = torch.relu(torch.cat((torch.matmul(adj, sup.detach()[..., :64]), sup.detach()[..., 64:]), dim=-1) + bias.detach())
    assert torch.allclose(kept["out"], want, rtol=1e-6, atol=1e-6) and sup.grad is not None and bias.grad is not None
    assert events == []


def test_the_head_issues_what_it_issued_and_equals_the_csr_kernel(gpu, meshes, monkeypatch):
    """zero_n_aggregate_head on the template: positions = base + scale * out[..., :3] out of the aggregation launch, the
    gradient [scale * grad_pos | 0] never materialised."""
    csr, scale = meshes["template"], 0.01
    g, sup, bias = _operands((B, 482, 192), gpu, 23)
    base = torch.randn(B, 482, 3, generator=g).to(gpu).requires_grad_(True)
    seed = torch.randn(B, 482, 3, generator=g).to(gpu)
    kept = {}

    def step():
        sup.grad = bias.grad = base.grad = None
        kept["pos"] = layers.zero_n_aggregate_head(sup, csr, bias, 64, F.relu, base, scale)
        kept["pos"].backward(seed)
        torch.cuda.synchronize()
    events = _entry_points(step, monkeypatch)
    _log("head-template-192", events)
    grad_out = torch.zeros(B, 482, 192, device=gpu)
    grad_out[..., :3] = scale * seed
    want_out, want_grad, ref, mass = _csr_kernel(csr, sup.detach(), bias.detach(), 64, F.relu, grad_out)
    assert torch.equal(kept["pos"], base.detach() + scale * want_out[..., :3])
    assert torch.equal(sup.grad, want_grad) and torch.equal(base.grad, seed)
    _bias_close(bias.grad, ref, mass)
    assert events == _expected("head-template-192")


def _stack_step(route, csr, gpu):
    """A three-layer 192-wide stack into positions, forward + backward under deferred parameter gradients."""
    torch.manual_seed(31)
    stack = [layers.Batch_Image_ZERON_GCNGCN(i, o).to(gpu) for i, o in ((48, 192), (192, 192), (192, 192))]
    g = torch.Generator(device="cpu").manual_seed(32)
    x = torch.randn(B, csr.nv, 48, generator=g).to(gpu).requires_grad_(True)
    base = torch.randn(B, csr.nv, 3, generator=g).to(gpu).requires_grad_(True)
    seed = torch.randn(B, csr.nv, 3, generator=g).to(gpu)
    leaves = [x, base] + [p for layer in stack for p in layer.parameters()]
    kept = {}

    def step():
        for p in leaves:
            p.grad = None
        with layers.deferred_parameter_gradients():
            if route == "layers":       # the layers one by one: the reference's call sequence
                h = x
                for layer in stack[:-1]:
                    h = layer(h, csr, F.relu)
                kept["pos"] = stack[-1].forward_positions(h, csr, F.relu, base, 0.01)
            else:
                kept["pos"] = layers.zero_n_stack_positions(x, csr, stack, F.relu, base, 0.01)
            kept["pos"].backward(seed)
        torch.cuda.synchronize()
    return step, kept, leaves


@pytest.mark.parametrize("force", [{"fwd": True, "bwd": True}, None], ids=["forced", "plan"])
def test_the_stack_head_issues_what_it_issued(gpu, meshes, monkeypatch, force):
    """Forced: the head's backward takes the product below it along (geom_zn_layer_bwd_f32), its column sums finish in the
    end-of-pass launch.  Un-forced at this small shard the plan says no: the separate head backward -- the very launches of
    the layers one by one, so the same bits; the boundary launches sum their products in another order (the bounds of
    tests/test_fused_layer_gpu.py: 2e-6 on positions, 2e-3 on gradients behind a ReLU that may switch)."""
    csr = meshes["sphere"]
    name = "stack-head-forced" if force else "stack-head-plan"
    step, kept, leaves = _stack_step("stack", csr, gpu)
    keep = fused.force
    fused.force = force
    try:
        events = _entry_points(step, monkeypatch)
    finally:
        fused.force = keep
    _log(name, events)
    got_pos, got = kept["pos"].detach().clone(), [p.grad.clone() for p in leaves]
    want_step, want_kept, want_leaves = _stack_step("layers", csr, gpu)
    want_step()
    want_pos, want = want_kept["pos"].detach(), [p.grad for p in want_leaves]
    if force is None:
        assert torch.equal(got_pos, want_pos)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    else:
        assert (got_pos - want_pos).abs().max().item() <= 2e-6 * want_pos.abs().max().item()
        for a, b in zip(got, want):
            assert (a - b).abs().max().item() <= 2e-3 * (b.abs().max().item() + 1e-30)
    assert events == _expected(name)


# Worked out from the host code, not yet recorded on a GPU (LAB_NOTES section 16).  A table
# entry point is called directly and its code checked (a refusal falls through to the CSR kernel's `call`); the head and the
# CSR kernel go through `_lib.call`.  At 324 rows every product of the stacks is the any-shape kernel's (geom_gemm_f32: forward, input gradient, weight
# gradient, in that order); a boundary's or the head's fused backward leaves the input gradient of the product below, so that
# product issues its weight gradient alone; the biases' column sums finish in the end-of-pass launch.
_TABLE = """
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
    """
_CSR = """
        call geom_zn_gcn_aggregate_fwd_f32
        check geom_zn_gcn_aggregate_fwd_f32
        call geom_zn_gcn_aggregate_bwd_f32
        check geom_zn_gcn_aggregate_bwd_f32
    """
ROUTES = {
    "relu-192": _TABLE, "elu-192": _TABLE, "none-192": _TABLE, "tanh-192": _TABLE, "any-width-300": _TABLE, "split10-40": _TABLE,
    "unbatched-192": _TABLE, "no-bias-192": _TABLE, "template-192": _TABLE, "no-table-192": _CSR, "no-table-7": _CSR,
    "head-template-192": """
        call geom_zn_gcn_aggregate_ell_head_fwd_f32
        check geom_zn_gcn_aggregate_ell_head_fwd_f32
        call geom_zn_gcn_aggregate_ell_head_bwd_f32
        check geom_zn_gcn_aggregate_ell_head_bwd_f32
    """,
    "stack-head-forced": """
        call geom_gemm_f32
        check geom_gemm_f32
        call geom_zn_layer_fwd_f32
        check geom_zn_layer_fwd_f32
        call geom_zn_layer_fwd_f32
        check geom_zn_layer_fwd_f32
        call geom_zn_gcn_aggregate_ell_head_fwd_f32
        check geom_zn_gcn_aggregate_ell_head_fwd_f32
        call geom_zn_layer_bwd_f32
        check geom_zn_layer_bwd_f32
        call geom_gemm_f32
        check geom_gemm_f32
        call geom_zn_layer_bwd_f32
        check geom_zn_layer_bwd_f32
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        call geom_gemm_f32
        check geom_gemm_f32
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
    "stack-head-plan": """
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        call geom_gemm_f32
        check geom_gemm_f32
        call geom_zn_gcn_aggregate_ell_head_fwd_f32
        check geom_zn_gcn_aggregate_ell_head_fwd_f32
        call geom_zn_gcn_aggregate_ell_head_bwd_f32
        check geom_zn_gcn_aggregate_ell_head_bwd_f32
        call geom_gemm_f32
        check geom_gemm_f32
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        call geom_gemm_f32
        check geom_gemm_f32
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        call geom_gemm_f32
        check geom_gemm_f32
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
}
