"""-m gpu: the narrow head (layers._NarrowHead: the last layer of a stack that ends in positions, computed on the three
columns that reach them) against the wide route it replaces, in the same process (`layers.narrow_head = "off"`): every tensor
that leaves the stack must carry the SAME BITS -- torch.equal throughout, no tolerance.  The wide route itself is pinned to
the CSR kernel, to float64 and to the oracle by tests/test_aggregate_route_gpu.py, test_fused_layer_gpu.py and test_dense_gpu.py.

Shapes: the smallest at which the new kernels can go wrong.  810 rows (5 x the 162-vertex icosphere) is above the pair
kernel's 512 and no multiple of 4, 16, 32, 48 or 64: a zero-filled last k-step of a split, ragged last tiles of both gradient
roles and a ragged last bias partial.  1446 rows (3 x the 482-vertex template): two 33-neighbour rows in the table's CSR
tail and an odd mesh count for the XCD assignment.  8 x 2562 rows: the workload's own row count, where the gate opens."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden
from geometrics_amd import _lib as L
from geometrics_amd import fused, layers, meshgen, optim, utils

pytestmark = pytest.mark.gpu

WIDTHS = ((48, 192), (192, 192), (192, 192))
NEW = ("geom_zn_gcn_narrow_head_fwd_f32", "geom_zn_gcn_narrow_head_bwd_f32", "geom_dense_bwd_narrow_f32")
WIDE_LAST = ("geom_zn_gcn_aggregate_ell_head_fwd_f32", "geom_zn_gcn_aggregate_ell_head_bwd_f32", "geom_dense_bwd_f32")


@pytest.fixture(scope="module")
def meshes(gpu):
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    csr = lambda faces: layers.adjacency_csr(utils.adj_init(to(faces))["adj"])
    sphere, template, big = csr(meshgen.icosphere(2)[1]), csr(golden("adj_482")["faces"]), csr(meshgen.icosphere(4)[1])
    assert sphere.nv == 162 and sphere.over is None
    assert template.nv == 482 and template.over is not None and template.over_t is not None
    assert big.nv == 2562
    return {"sphere": (sphere, 5), "template": (template, 3), "big": (big, 8)}


@contextlib.contextmanager
def _mode(mode):
    keep, layers.narrow_head = layers.narrow_head, mode
    try:
        yield
    finally:
        layers.narrow_head = keep


def _problem(mesh, gpu, widths=WIDTHS):
    csr, b = mesh
    torch.manual_seed(41)
    stack = [layers.Batch_Image_ZERON_GCNGCN(i, o).to(gpu) for i, o in widths]
    g = torch.Generator(device="cpu").manual_seed(42 + csr.nv)
    x = torch.randn(b, csr.nv, widths[0][0], generator=g).to(gpu).requires_grad_(True)
    base = torch.randn(b, csr.nv, 3, generator=g).to(gpu).requires_grad_(True)
    seed = torch.randn(b, csr.nv, 3, generator=g).to(gpu)
    return csr, stack, x, base, seed


def _names(stack):
    return ["pos", "x.grad", "base.grad"] + ["%s%d.grad" % (n, i) for i in range(len(stack)) for n in ("weight", "bias")]


def _pass(mode, mesh, gpu, activation, deferred, widths=WIDTHS):
    """One forward + backward of a fresh stack: [positions, x.grad, base.grad, weight1.grad and bias.grad of every layer]."""
    csr, stack, x, base, seed = _problem(mesh, gpu, widths)
    with _mode(mode), (layers.deferred_parameter_gradients() if deferred else contextlib.nullcontext()):
        pos = layers.zero_n_stack_positions(x, csr, stack, activation, base, 0.01)
        pos.backward(seed)
    torch.cuda.synchronize()
    return [pos.detach(), x.grad, base.grad] + [p.grad for layer in stack for p in (layer.weight1, layer.bias)]


_wide = {}


def _wide_pass(name, meshes, gpu, activation, deferred):
    """The wide route's pass, computed once per case and shared."""
    key = (name, activation, deferred)
    if key not in _wide:
        _wide[key] = _pass("off", meshes[name], gpu, activation, deferred)
    return _wide[key]


def _assert_equal(got, want, names):
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and torch.equal(a, b), "%s differs: %d of %d elements, max |diff| %.3e" % (
            name, int((a != b).sum()), a.numel(), float((a - b).abs().max()))


@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "immediate"])
@pytest.mark.parametrize("activation", [F.relu, None], ids=["relu", "none"])
@pytest.mark.parametrize("name", ["sphere", "template"])
def test_every_tensor_equals_the_wide_route_and_the_dead_columns_are_zero(gpu, meshes, name, activation, deferred):
    want = _wide_pass(name, meshes, gpu, activation, deferred)
    got = _pass("on", meshes[name], gpu, activation, deferred)
    assert all(bool(torch.isfinite(t).all()) for t in want)
    assert float(want[1].abs().max()) > 0 and float(want[-2][..., :3].abs().max()) > 0
    _assert_equal(got, want, _names(WIDTHS))
    w3, b3 = got[-2], got[-1]
    assert w3.shape == (1, 192, 192) and not bool(w3[..., 3:].any()) and not bool(b3[3:].any())


@pytest.mark.parametrize("name", ["sphere", "template"])
def test_forward_without_gradient_equals_the_forward_with(gpu, meshes, name):
    csr, stack, x, base, _ = _problem(meshes[name], gpu)
    with _mode("on"):
        with torch.no_grad():
            plain = layers.zero_n_stack_positions(x, csr, stack, F.relu, base, 0.01)
        tracked = layers.zero_n_stack_positions(x, csr, stack, F.relu, base, 0.01)
    assert tracked.requires_grad and not plain.requires_grad
    assert torch.equal(plain, tracked.detach())
    assert torch.equal(plain, _wide_pass(name, meshes, gpu, F.relu, True)[0])


def _adam_step(mode, mesh, gpu):
    csr, stack, x, base, seed = _problem(mesh, gpu)
    opt = optim.FusedAdam([p for layer in stack for p in layer.parameters()], lr=1e-3)
    with _mode(mode), layers.deferred_parameter_gradients(), opt.in_backward():
        layers.zero_n_stack_positions(x, csr, stack, F.relu, base, 0.01).backward(seed)
        stepped = bool(opt._stepped_in_backward)
    torch.cuda.synchronize()
    return stepped, [p.detach() for p in opt.params] + list(opt.exp_avg) + list(opt.exp_avg_sq)


def test_adam_still_rides_in_the_end_of_pass_launch(gpu, meshes):
    fresh = [p.detach().clone() for layer in _problem(meshes["sphere"], gpu)[1] for p in layer.parameters()]
    wide_stepped, want = _adam_step("off", meshes["sphere"], gpu)
    narrow_stepped, got = _adam_step("on", meshes["sphere"], gpu)
    assert wide_stepped and narrow_stepped
    assert not torch.equal(want[4], fresh[4])          # (the last layer's weight did move)
    names = ["%s %d" % (kind, i) for kind in ("parameter", "exp_avg", "exp_avg_sq") for i in range(6)]
    _assert_equal(got, want, names)


def test_a_captured_pass_follows_a_weight_overwritten_in_place(gpu, meshes):
    csr, stack, x, base, seed = _problem(meshes["sphere"], gpu)
    leaves = [x, base] + [p for layer in stack for p in layer.parameters()]
    kept = {}

    def step():
        for p in leaves:
            p.grad = None
        kept["pos"] = layers.zero_n_stack_positions(x, csr, stack, F.relu, base, 0.01)
        kept["pos"].backward(seed)

    with _mode("on"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        old_pos = kept["pos"].detach().clone()
        g = torch.Generator(device="cpu").manual_seed(77)
        new_w = (torch.rand(1, 192, 192, generator=g) - 0.5).mul_(0.4).to(gpu)
        with torch.no_grad():
            stack[-1].weight1.copy_(new_w)
        graph.replay()
        torch.cuda.synchronize()
    got = [kept["pos"].detach()] + [p.grad for p in leaves]
    # an eager pass of the wide route on the new weight
    _, stack2, x2, base2, _ = _problem(meshes["sphere"], gpu)
    with torch.no_grad():
        stack2[-1].weight1.copy_(new_w)
    with _mode("off"):
        pos2 = layers.zero_n_stack_positions(x2, csr, stack2, F.relu, base2, 0.01)
        pos2.backward(seed)
    torch.cuda.synchronize()
    want = [pos2.detach(), x2.grad, base2.grad] + [p.grad for layer in stack2 for p in layer.parameters()]
    assert not torch.equal(old_pos, want[0])
    _assert_equal(got, want, _names(WIDTHS))


def _issued(step, monkeypatch):
    """The entry points the second call of step() issues: the names handed to _lib.status, through which _lib.call goes too."""
    step()
    names = []
    real_status = L.status

    def status_spy(name, *args, **kwargs):
        names.append(name)
        return real_status(name, *args, **kwargs)
    with monkeypatch.context() as m:
        m.setattr(L, "status", status_spy)
        step()
    return names


def _stepper(mode, mesh, gpu, activation=F.relu, force=None):
    csr, stack, x, base, seed = _problem(mesh, gpu)
    leaves = [x, base] + [p for layer in stack for p in layer.parameters()]
    kept = {}

    def step():
        for p in leaves:
            p.grad = None
        keep_force, fused.force = fused.force, force
        try:
            with _mode(mode), layers.deferred_parameter_gradients():
                kept["pos"] = layers.zero_n_stack_positions(x, csr, stack, activation, base, 0.01)
                kept["pos"].backward(seed)
        finally:
            fused.force = keep_force
        torch.cuda.synchronize()
    return step, lambda: [kept["pos"].detach()] + [p.grad for p in leaves]


@pytest.mark.parametrize("name", ["sphere", "template"])
def test_the_gate_keeps_the_small_shapes_on_their_launches(gpu, meshes, monkeypatch, name):
    step, _ = _stepper(None, meshes[name], gpu)
    names = _issued(step, monkeypatch)
    assert not set(names) & set(NEW)
    assert set(WIDE_LAST) <= set(names)


def test_the_gate_opens_at_the_workload_row_count(gpu, meshes, monkeypatch):
    assert 8 * 2562 >= layers.NARROW_HEAD_MIN_ROWS >= 4096
    step, results = _stepper(None, meshes["big"], gpu)
    names = _issued(step, monkeypatch)
    assert set(NEW) <= set(names)
    assert "geom_zn_gcn_aggregate_ell_head_fwd_f32" not in names and "geom_zn_gcn_aggregate_ell_head_bwd_f32" not in names
    assert names.count("geom_dense_bwd_narrow_f32") == 1
    got = results()
    wide_step, wide_results = _stepper("off", meshes["big"], gpu)
    wide_names = _issued(wide_step, monkeypatch)
    assert not set(wide_names) & set(NEW) and set(WIDE_LAST) <= set(wide_names)
    # the pair launches of the layers below stay; the last layer's is the one the narrow route replaces
    assert wide_names.count("geom_dense_bwd_f32") == names.count("geom_dense_bwd_f32") + 1 == 3
    _assert_equal(got, wide_results(), _names(WIDTHS))


@pytest.mark.parametrize("case", ["elu", "forced-boundary"])
def test_what_the_narrow_route_does_not_take_is_untouched(gpu, meshes, monkeypatch, case):
    activation = F.elu if case == "elu" else F.relu
    force = {"fwd": True, "bwd": True} if case == "forced-boundary" else None
    on_step, on_results = _stepper("on", meshes["sphere"], gpu, activation, force)
    names = _issued(on_step, monkeypatch)
    assert not set(names) & set(NEW)
    off_step, off_results = _stepper("off", meshes["sphere"], gpu, activation, force)
    assert _issued(off_step, monkeypatch) == names
    _assert_equal(on_results(), off_results(), _names(WIDTHS))


def test_a_single_layer_whose_input_needs_no_gradient(gpu, meshes, monkeypatch):
    """forward_positions on features that need no gradient: the narrow pair launch runs its weight-gradient role alone, where the
    wide route runs the split launch alone."""
    csr, b = meshes["sphere"]
    results = {}
    for mode in ("off", "on"):
        torch.manual_seed(43)
        layer = layers.Batch_Image_ZERON_GCNGCN(192, 192).to(gpu)
        g = torch.Generator(device="cpu").manual_seed(44)
        x = torch.randn(b, csr.nv, 192, generator=g).to(gpu)
        base = torch.randn(b, csr.nv, 3, generator=g).to(gpu)
        seed = torch.randn(b, csr.nv, 3, generator=g).to(gpu)
        kept = {}

        def step():
            layer.weight1.grad = layer.bias.grad = None
            with _mode(mode):
                kept["pos"] = layer.forward_positions(x, csr, F.relu, base, 0.01)
                kept["pos"].backward(seed)
            torch.cuda.synchronize()
        names = _issued(step, monkeypatch)
        assert ("geom_dense_bwd_narrow_f32" in names) == (mode == "on") and ("geom_dense_bwd_weight_f32" in names) == (mode == "off")
        results[mode] = [kept["pos"].detach(), layer.weight1.grad, layer.bias.grad]
    assert float(results["off"][1].abs().max()) > 0
    _assert_equal(results["on"], results["off"], ["pos", "weight1.grad", "bias.grad"])
