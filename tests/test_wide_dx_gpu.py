"""-m gpu: the wide first layer's input gradient dX = G . W^T on the bf16 matrix cores (csrc/dense_dx_split_bf16.hip,
dense.backward_input_split): exact fp32 products, a fixed-order fp32 sum.  Shapes are the smallest at which the kernel can go
wrong: rows 3 (less than a 16-row block), 83 (a ragged block), 179, 1297 (more row-blocks than one workgroup keeps, so several
workgroups, plus a stray row); cin 193 (one valid column in the last 16-column tile), 208 (no ragged tile), 963 and 1155 (three
valid columns in the last tile, rows of dX only 4-byte aligned)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from geometrics_amd import dense, layers, meshgen, products, utils
from oracle import ref_ops

pytestmark = pytest.mark.gpu

ROWS = (3, 83, 179, 1297)
CINS = (193, 208, 963, 1155)
K = 192


@pytest.fixture
def forced(monkeypatch):
    """The kernel wherever it takes the operands, whatever the row count."""
    monkeypatch.setattr(dense, "wide_dx", "split")


@functools.lru_cache(maxsize=None)
def _random_case(rows, cin):
    """(g, w, dx of the kernel, exact float64 product, float64 mass) on the device / host: computed once, read by several tests."""
    gen = torch.Generator().manual_seed(1000 * rows + cin)
    g = torch.randn(rows, K, generator=gen).cuda()
    w = (torch.randn(cin, K, generator=gen) * 0.05).cuda()
    dx = dense.backward_input_split(g, w)
    g64, w64 = g.double().cpu(), w.double().cpu()
    return g, w, dx, g64 @ w64.t(), g64.abs() @ w64.abs().t()


def _planes_value(planes):
    """bf16 bit patterns (int16) -> float64 values."""
    bits = planes.cpu().numpy().astype(np.uint16).astype(np.uint32) << 16
    return bits.view(np.float32).astype(np.float64)


@pytest.mark.parametrize("cin", CINS)
def test_planes_sum_to_the_weight_exactly_and_their_padding_is_zero(gpu, cin):
    torch.manual_seed(cin)
    w = torch.randn(cin, K, device=gpu) * 0.05
    planes = dense.wide_dx_planes_matrix(dense.wide_dx_planes(w))
    assert planes.shape[0] == 3 and planes.shape[2] == K and planes.shape[1] >= cin and planes.shape[1] % 16 == 0
    v = _planes_value(planes)
    assert np.array_equal((v[0] + v[1] + v[2])[:cin], w.cpu().numpy().astype(np.float64))
    assert float(np.abs(v[:, cin:]).max(initial=0.0)) == 0.0
    assert float(np.abs(v[1]).max()) <= 2.0 ** -8 * float(np.abs(v[0]).max())      # the planes are the three bf16 digits


# more row-blocks than compute units, by a few: the launch hands the stray row-blocks out a column group per workgroup
STRAY = [(4100, 193), (4100, 963)]


@pytest.mark.parametrize("rows,cin", [(r, c) for c in CINS for r in ROWS] + STRAY)
def test_small_integer_operands_give_the_integer_product_bit_for_bit(gpu, rows, cin):
    """|v| <= 8 integers: every partial sum is an integer below 2^24, so wrong planes, indices or ragged tiles show without a
    tolerance.  Asymmetric operands (a transposed tile cannot pass)."""
    gen = torch.Generator().manual_seed(7 * rows + cin)
    g = torch.randint(-8, 9, (rows, K), generator=gen).float()
    w = torch.randint(-8, 9, (cin, K), generator=gen).float()
    expect = (g.double() @ w.double().t()).float()
    got = dense.backward_input_split(g.to(gpu), w.to(gpu)).cpu()
    assert torch.equal(got, expect)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("cin", CINS)
def test_one_hot_rows_return_the_weight_columns_exactly(gpu, rows, cin):
    """Row r of g = e_k: output row r is w[:, k] to the bit -- all three planes arrive and recombine."""
    gen = torch.Generator().manual_seed(rows + 13 * cin)
    w = torch.randn(cin, K, generator=gen) * 0.05
    ks = torch.randint(0, K, (rows,), generator=gen)
    ks[: min(rows, 3)] = torch.tensor([0, K - 1, 37])[: min(rows, 3)]
    g = torch.zeros(rows, K)
    g[torch.arange(rows), ks] = 1.0
    got = dense.backward_input_split(g.to(gpu), w.to(gpu)).cpu()
    assert torch.equal(got, w[:, ks].t().contiguous())


@pytest.mark.parametrize("rows,cin", [(r, c) for c in CINS for r in ROWS] + STRAY)
def test_no_further_from_float64_than_the_native_fp32_product(gpu, rows, cin):
    """The promotion rule of tests/test_split_bf16_gpu.py: every element inside (k + 8) 2^-24 sum|g||w|; from 179 rows on (a
    sample large enough for the statistics) the rms error within 1.05 x and the worst error over mass within 1.5 x of the
    native fp32 product's on the same inputs."""
    g, w, dx, exact, mass = _random_case(rows, cin)
    assert bool(torch.isfinite(dx).all())
    err = (dx.double().cpu() - exact).abs()
    assert bool((err <= (K + 8) * 2.0 ** -24 * mass + 1e-30).all())
    native = torch.mm(g, w.t())
    err_native = (native.double().cpu() - exact).abs()
    rms = lambda e: float(e.pow(2).mean().sqrt())
    print("rows %d cin %d: rms error split %.3e native %.3e; worst / mass split %.3e native %.3e"
          % (rows, cin, rms(err), rms(err_native), float((err / mass).max()), float((err_native / mass).max())))
    if rows >= 179:
        assert rms(err) <= rms(err_native) * 1.05, (rms(err), rms(err_native))
        assert float((err / mass).max()) <= float((err_native / mass).max()) * 1.5


@pytest.mark.parametrize("rows,cin", [(3, 193), (83, 963), (179, 1155), (1297, 963)])
def test_nothing_outside_the_output_is_written(gpu, rows, cin):
    """dx as a view inside a sentinel-filled buffer: guards before, after and between the rows."""
    g, w, dx, _, _ = _random_case(rows, cin)
    pitch, lead = cin + 5, 1031
    sentinel = -12345.678
    buf = torch.full((lead + rows * pitch + 977,), sentinel, device=gpu)
    view = buf[lead:lead + rows * pitch].view(rows, pitch)[:, :cin]
    out = dense.backward_input_split(g, w, out=view)
    assert out.data_ptr() == view.data_ptr() and torch.equal(view, dx)
    guard = torch.ones_like(buf, dtype=torch.bool)
    guard[lead:lead + rows * pitch].view(rows, pitch)[:, :cin] = False
    assert bool((buf[guard] == sentinel).all())


@pytest.mark.parametrize("rows,cin", [(1297, 193), (1297, 963)] + STRAY)
def test_same_bits_twice_and_whichever_rows_share_the_call(gpu, rows, cin):
    g, w, dx, _, _ = _random_case(rows, cin)
    assert torch.equal(dense.backward_input_split(g, w), dx)
    for a, b in ((0, 3), (16, 99), (83, 1297), (1280, 1297), (640, 641), (rows - 21, rows)):
        assert torch.equal(dense.backward_input_split(g[a:b], w), dx[a:b]), (a, b)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_a_non_finite_row_stays_in_its_row(gpu, bad):
    g, w, dx, _, _ = _random_case(179, 963)
    g2 = g.clone()
    g2[77, 5] = bad
    got = dense.backward_input_split(g2, w)
    assert not bool(torch.isfinite(got[77]).any())
    keep = torch.arange(179, device=gpu) != 77
    assert torch.equal(got[keep], dx[keep])


def _stack(gpu):
    torch.manual_seed(31)
    V, Fc = meshgen.icosphere(3)
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    stack = torch.nn.ModuleList([layers.Batch_Image_ZERON_GCNGCN(963, 192), layers.Batch_Image_ZERON_GCNGCN(192, 192)]).to(gpu)
    x = torch.randn(2, V.shape[0], 963, device=gpu, requires_grad=True)
    g_out = torch.randn(2, V.shape[0], 192, device=gpu)
    return adj, stack, x, g_out


def test_through_the_layers_immediate_and_postponed(gpu, forced, monkeypatch):
    """963 -> 192 -> 192 on icosphere(3), 2 meshes, the kernel forced on: x.grad against the float64 restatement at the bound
    tests/test_ops_parity_gpu.py holds the same stack to (1e-4 of the gradient's scale), the immediate and the postponed
    (late_input_gradients) products bit-identical -- and both really ran on the kernel."""
    adj, stack, x, g_out = _stack(gpu)
    ran = []
    real = dense.backward_input_split
    monkeypatch.setattr(dense, "backward_input_split", lambda *a, **k: (ran.append(tuple(a[0].shape)), real(*a, **k))[1])

    def run(late):
        x.grad = None
        for p_ in stack.parameters():
            p_.grad = None
        with layers.deferred_parameter_gradients(), layers.late_input_gradients(enabled=late):
            stack[1](stack[0](x, adj, F.elu), adj, F.elu).backward(g_out)
        return x.grad.clone()

    now, late = run(False), run(True)
    assert ran == [(2 * 642, 192)] * 2
    assert torch.equal(now, late)
    xc = x.detach().cpu().double().requires_grad_(True)
    hc = xc
    for l in stack:
        hc = ref_ops.zero_n_layer(hc, adj.cpu().double(), l.weight1.detach().cpu().double(), l.bias.detach().cpu().double(), 3, F.elu)
    hc.backward(g_out.cpu().double())
    ref = xc.grad.numpy()
    assert np.abs(now.cpu().numpy().astype(np.float64) - ref).max() <= 1e-4 * np.abs(ref).max()


def test_a_replayed_graph_follows_the_weight_it_is_replayed_on(gpu, forced):
    """The stale-planes trap: the planes are made inside every call, so a captured backward re-splits the weight it finds."""
    torch.manual_seed(5)
    layer = layers.Batch_Image_ZERON_GCNGCN(963, 192).to(gpu)
    w = layer.weight1
    g = torch.randn(179, K, device=gpu)
    out = torch.empty(179, 963, device=gpu)
    w2 = w.detach().view(963, K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        products._input_gradient("lib", g, w2, out=out)        # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        products._input_gradient("lib", g, w2, out=out)
    graph.replay()
    first = out.clone()
    assert torch.equal(first, dense.backward_input_split(g, w2))
    with torch.no_grad():
        w.mul_(-1.5).add_(0.01)
    graph.replay()
    assert torch.equal(out, dense.backward_input_split(g, w2)) and not torch.equal(out, first)


def test_the_default_leaves_small_products_with_the_library(gpu, monkeypatch):
    """648 rows against the 963-wide layer: below the threshold nothing is launched on the kernel by default."""
    monkeypatch.setattr(dense, "wide_dx", None)
    monkeypatch.delenv("GEOM_WIDE_DX", raising=False)
    ran = []
    real = dense.backward_input_split
    monkeypatch.setattr(dense, "backward_input_split", lambda *a, **k: (ran.append(tuple(a[0].shape)), real(*a, **k))[1])
    torch.manual_seed(9)
    V, Fc = meshgen.icosphere(2)
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    layer = layers.Batch_Image_ZERON_GCNGCN(963, 192).to(gpu)
    x = torch.randn(4, V.shape[0], 963, device=gpu, requires_grad=True)
    g_out = torch.randn(4, V.shape[0], 192, device=gpu)
    layer(x, adj, F.relu).backward(g_out)
    lib = x.grad.clone()
    assert ran == [] and not dense.wide_dx_plan(648, 963, 192) and dense.wide_dx_plan(20496, 963, 192)
    monkeypatch.setattr(dense, "wide_dx", "split")
    x.grad = None
    layer(x, adj, F.relu).backward(g_out)
    assert ran == [(648, 192)]
    assert float((x.grad - lib).abs().max()) <= 1e-5 * float(lib.abs().max())
    monkeypatch.setattr(dense, "wide_dx", "lib")
    x.grad = None
    layer(x, adj, F.relu).backward(g_out)
    assert ran == [(648, 192)] and torch.equal(x.grad, lib)
