"""-m gpu: the three aggregation kernels of csrc/zn_gcn.hip through the C ABI, on what no other test reaches -- a WIDTH-16
neighbour table (meshgen.hub_ring_adjacency: 70 vertices, hub rows of 41 and 27 entries, so 25 and 11 entries in the CSR tail:
more than one tail round at either round size) next to the width-8 table of the 482-vertex template (33-entry poles), at
vertex counts that are no multiple of any kernel's rows per workgroup (ragged last tile; in the backward a second row tile
that is partly or wholly empty).

* the table kernels (split 3 with the sign mask and the head, split 10, any width at VEC 4 / 2 / 1) carry the BITS of the CSR
  kernel on the same operands: same neighbour order, same sum;
* the bias gradient (another partial layout per kernel) against float64 with the bound of tests/test_aggregate_any_gpu.py,
  exactly geom_zn_gcn_bwd_partial_rows rows written, the NaN-prefilled scratch beyond them untouched;
* the CSR kernel itself against a float64 dense restatement, with test_long_rows_take_the_ell_kernel_with_a_csr_tail's bound."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import golden
from geometrics_amd import _lib as L
from geometrics_amd import layers, meshgen, utils

pytestmark = pytest.mark.gpu

B, SCALE = 2, 0.01
NAN = float("nan")
ACTS = (0, 1, 2)                     # none, ReLU, ELU
FAST3, FAST10, ANY = (72, 24), (120, 12), [(52, 6), (50, 5), (7, 3)]
# (c, k, activation, where the backward takes act' from: the saved output, the sign mask, or head mode)
TABLE_CASES = ([FAST3 + (act, "saved") for act in ACTS] + [FAST3 + (1, "mask"), FAST3 + (1, "head"), FAST3 + (0, "head")]
               + [FAST10 + (act, "saved") for act in ACTS] + [shape + (act, "saved") for shape in ANY for act in ACTS])
CSR_CASES = [shape + (act,) for shape in [FAST3, FAST10] + ANY for act in ACTS]


@pytest.fixture(scope="module")
def graphs(gpu):
    """name -> (CSR with its tables, the dense adjacency)."""
    wide = torch.from_numpy(meshgen.hub_ring_adjacency()).to(gpu)
    template = utils.adj_init(torch.from_numpy(np.ascontiguousarray(golden("adj_482")["faces"])).to(gpu))["adj"]
    out = {}
    for name, dense, width, longest in (("wide16", wide, 16, 41), ("template", template, 8, 33)):
        csr = layers.adjacency_csr(dense)
        assert csr.ell_w == width and csr.over is not None and csr.over_t is not None
        assert int((csr.rowptr[1:] - csr.rowptr[:-1]).max()) == longest
        assert not torch.equal(dense, dense.t())
        out[name] = (csr, dense)
    assert out["wide16"][0].nv == 70 and out["template"][0].nv == 482
    return out


def _csr_backward(csr, c, k, act, gout, saved):
    """geom_zn_gcn_aggregate_bwd_f32 -> (input gradient, bias gradient, NaN-prefilled scratch)."""
    b, nv = gout.shape[:2]
    grad, gb = torch.full_like(gout, NAN), torch.full((c,), NAN, device=gout.device)
    scr = torch.full((L.lib().geom_zn_gcn_bwd_scratch_floats(b, nv, c),), NAN, device=gout.device)
    L.call("geom_zn_gcn_aggregate_bwd_f32", b, nv, c, k, csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(), csr.val_t.data_ptr(),
           gout.data_ptr(), L.ptr(saved), act, grad.data_ptr(), gb.data_ptr(), scr.data_ptr())
    return grad, gb, scr


@pytest.fixture(scope="module")
def csr_kernel(gpu, graphs):
    """(graph, c, k, act) -> seeded operands and what the CSR kernel makes of them; computed once, shared, never written."""
    memo = {}

    def get(graph, c, k, act):
        key = (graph, c, k, act)
        if key not in memo:
            csr = graphs[graph][0]
            g = torch.Generator(device="cpu").manual_seed(1000 * c + 10 * k + act)
            sup, bias, gout = (torch.randn(*s, generator=g).to(gpu) for s in ((B, csr.nv, c), (c,), (B, csr.nv, c)))
            out = torch.full_like(sup, NAN)
            L.call("geom_zn_gcn_aggregate_fwd_f32", B, csr.nv, c, k, csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(),
                   sup.data_ptr(), bias.data_ptr(), act, out.data_ptr())
            grad, gb, scr = _csr_backward(csr, c, k, act, gout, out if act else None)
            memo[key] = SimpleNamespace(sup=sup, bias=bias, gout=gout, out=out, grad=grad, gb=gb, scr=scr)
        return memo[key]
    return get


def _with_derivative(gout, out, act):
    """g' = g * act'(out) in float64, act' read from the kernel's fp32 output the way the kernels read it."""
    gp = gout.double()
    if act == 1:
        gp = gp * (out > 0)
    elif act == 2:
        gp = torch.where(out > 0, gp, gp * (out.double() + 1))
    return gp


def _check_bias_gradient(gb, scr, gp, rows):
    """Column sums of g' against float64 within 1e-6 of the column's mass -- the reduced gradient and the raw partial rows --
    with exactly `rows` rows written and the NaN-prefilled scratch beyond them untouched."""
    c = gp.shape[-1]
    ref, mass = gp.view(-1, c).sum(0), gp.abs().view(-1, c).sum(0)
    err = (gb.double() - ref).abs()
    print("bias gradient: worst |err| / mass %.3g (bound 1e-6)" % float((err / (mass + 1e-30)).max()))
    assert bool((err <= 1e-6 * mass + 1e-30).all())
    assert rows > 0 and rows * c <= scr.numel()
    part = scr[:rows * c].view(rows, c)
    assert not bool(torch.isnan(part).any()) and (rows * c == scr.numel() or bool(torch.isnan(scr[rows * c:]).all()))
    assert bool(((part.double().sum(0) - ref).abs() <= 1e-6 * mass + 1e-30).all())


def _sign_bits(out, k):
    """out > 0 in the sign mask's layout: word (row, j), bit 4 * i + e <-> out[row, k * i + 4 * j + e]."""
    b, nv, _ = out.shape
    return (out > 0).view(b, nv, 3, k // 4, 4).permute(0, 1, 3, 2, 4).reshape(b, nv, k // 4, 12).int()


@pytest.mark.parametrize("graph", ["wide16", "template"])
@pytest.mark.parametrize("c,k,act,mode", TABLE_CASES, ids=["%d-%d-act%d-%s" % case for case in TABLE_CASES])
def test_table_kernels_carry_the_csr_kernels_bits(gpu, graphs, csr_kernel, graph, c, k, act, mode):
    csr, want = graphs[graph][0], csr_kernel(graph, c, k, act)
    nv, w = csr.nv, csr.ell_w
    table = (csr.ell_col.data_ptr(), csr.ell_val.data_ptr()) + tuple(t.data_ptr() for t in csr.over)
    table_t = (csr.ell_col_t.data_ptr(), csr.ell_val_t.data_ptr()) + tuple(t.data_ptr() for t in csr.over_t)
    masked = mode == "mask" or (mode == "head" and act == 1)
    mask = torch.zeros(L.lib().geom_zn_gcn_relu_mask_words(B, nv, c, k), dtype=torch.int16, device=gpu) if masked else None
    assert mask is None or mask.numel() == B * nv * (k // 4)
    out = torch.full_like(want.sup, NAN)
    # ---- forward
    if mode == "head":
        g = torch.Generator(device="cpu").manual_seed(c + k + act)
        base, grad_pos = torch.randn(B, nv, 3, generator=g).to(gpu), torch.randn(B, nv, 3, generator=g).to(gpu)
        pos = torch.full_like(base, NAN)
        L.call("geom_zn_gcn_aggregate_ell_head_fwd_f32", B, nv, c, k, w, *table, want.sup.data_ptr(), want.bias.data_ptr(), act,
               out.data_ptr(), L.ptr(mask), base.data_ptr(), SCALE, pos.data_ptr())
        assert torch.equal(pos, base + SCALE * want.out[..., :3])
    else:
        L.call("geom_zn_gcn_aggregate_ell_fwd_f32", B, nv, c, k, w, *table, want.sup.data_ptr(), want.bias.data_ptr(), act,
               out.data_ptr(), L.ptr(mask))
    assert torch.equal(out, want.out)
    if masked:
        bits = (mask.view(B, nv, k // 4, 1).int() >> torch.arange(12, device=gpu).int()) & 1
        assert torch.equal(bits, _sign_bits(want.out, k))
    # ---- backward
    grad, gb = torch.full_like(want.sup, NAN), torch.full((c,), NAN, device=gpu)
    scr = torch.full_like(want.scr, NAN)
    saved = want.out if (act and not masked) else None
    if mode == "head":       # the plain backward fed [scale * grad_pos | 0] is the statement of what the head's computes
        gout = torch.zeros_like(want.sup)
        gout[..., :3] = SCALE * grad_pos
        want_grad = _csr_backward(csr, c, k, act, gout, want.out if act else None)[0]
        L.call("geom_zn_gcn_aggregate_ell_head_bwd_f32", B, nv, c, k, w, *table_t, grad_pos.data_ptr(), SCALE, L.ptr(mask), act,
               grad.data_ptr(), gb.data_ptr(), scr.data_ptr())
    else:
        gout, want_grad = want.gout, want.grad
        L.call("geom_zn_gcn_aggregate_ell_bwd_f32", B, nv, c, k, w, *table_t, gout.data_ptr(), L.ptr(saved), L.ptr(mask), act,
               grad.data_ptr(), gb.data_ptr(), scr.data_ptr())
    assert torch.equal(grad, want_grad)
    _check_bias_gradient(gb, scr, _with_derivative(gout, want.out, act), int(L.lib().geom_zn_gcn_bwd_partial_rows(B, nv, c, k, w)))


def _close(actual, expected, rtol, what):
    """tests/test_ops_parity_gpu.py's max-norm closeness: |actual - expected| <= rtol * max|expected|, element-wise."""
    err, scale = float((actual.double() - expected).abs().max()), float(expected.abs().max())
    print("%s: max |err| / max |expected| %.3g (bound %g)" % (what, err / max(scale, 1e-30), rtol))
    assert err <= rtol * max(scale, 1e-30)


@pytest.mark.parametrize("graph", ["wide16", "template"])
@pytest.mark.parametrize("c,k,act", CSR_CASES)
def test_csr_kernel_equals_the_float64_dense_restatement(gpu, graphs, csr_kernel, graph, c, k, act):
    """cat(A . S[..., :k], S[..., k:]) + bias and its adjoint in float64.  ELU and no activation: forward and backward as they
    stand; ReLU: the backward alone, relu' from the kernel's own output (no knife edges)."""
    (csr, dense), got = graphs[graph], csr_kernel(graph, c, k, act)
    a, s = dense.double(), got.sup.double()
    out = torch.cat((torch.matmul(a, s[..., :k]), s[..., k:]), -1) + got.bias.double()
    if act == 2:
        out = torch.nn.functional.elu(out)
    if act != 1:
        _close(got.out, out, 1e-5, "output")
    gp = _with_derivative(got.gout, got.out if act == 1 else out, act)
    _close(got.grad, torch.cat((torch.matmul(a.t(), gp[..., :k]), gp[..., k:]), -1), 1e-5, "input gradient")
    _check_bias_gradient(got.gb, got.scr, _with_derivative(got.gout, got.out, act),
                         int(L.lib().geom_zn_gcn_bwd_partial_rows(B, csr.nv, c, k, 0)))
