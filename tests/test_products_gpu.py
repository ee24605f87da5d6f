"""-m gpu: which kernels a layer's product `support = input @ W` and its two gradients run on (geometrics_amd/products.py).

* the route pin: what one warmed-up forward + backward issues -- the library entry points through `_lib.call` / `_lib.check`,
  the `dense.*` wrappers, and `torch.matmul` / `torch.mm` / `torch.bmm` as the product module sees them, each with its operand
  shapes, in order -- against lists recorded from the code as it was when three autograd nodes and six predicates made these
  decisions (`GEOM_ROUTE_LOG=file` writes what a run issues).  One shape per route, each under a plain backward, under deferred
  parameter gradients with a postponed input gradient, inside weight_gradient_batching(), across two fused layer boundaries,
  and all of it again with the package's own products preferred over the library's;
* a differentiable product whose forward runs on a kernel of this package has its gradients, against float64."""
import os

import pytest
import torch
import torch.nn.functional as F

from geometrics_amd import _lib, dense, fused, layers, meshgen, products, utils
from test_dense_gpu import _rows_close

pytestmark = pytest.mark.gpu

# batch (of 162-vertex meshes), cin, c: one per route of products.route()
SHAPES = [(4, 48, 48),      # 648 rows: input and weight gradient in one launch
          (4, 99, 48),      # the split weight gradient alone (cin % 4)
          (4, 196, 48),     # the same (cin > 192)
          (4, 40, 40),      # the any-shape kernel
          (2, 48, 48),      # the same: 324 rows are too few for the 192-column kernels
          (4, 48, 16),      # the same; the package's own forward once the any-shape kernel is switched off
          (1, 48, 48),      # 162 rows: the library alone
          (4, 192, 3)]      # the any-shape kernel (a coordinate head)
MODES = ["plain", "late", "batched", "stack"]
CASES = [("%dx%d->%d" % (162 * b, cin, c), mode, b, cin, c) for b, cin, c in SHAPES for mode in MODES[:2]] \
    + [("648x99->48 + 3x(648x48->48)", "batched", 4, 48, 48), ("3x(648x192->192)", "stack", 4, 192, 192)]


@pytest.fixture(scope="module")
def mesh(gpu):
    V, Fc = meshgen.icosphere(2)
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    return V.shape[0], adj, layers.adjacency_csr(adj)


def _describe(name, args, kwargs):
    parts = [name]
    for a in args:
        if torch.is_tensor(a):
            parts.append("x".join(map(str, a.shape)))
    for key in sorted(kwargs):
        value = kwargs[key]
        if torch.is_tensor(value):
            parts.append("%s=%s" % (key, "x".join(map(str, value.shape))))
        elif value is not None and value is not False:
            parts.append("%s=%s" % (key, value))
    return " ".join(parts)


class _TorchAsSeen:
    """The torch module with its three product functions recorded: put in place of a module's global `torch`."""
    def __init__(self, events):
        for name in ("matmul", "mm", "bmm"):
            setattr(self, name, self._spy(name, events))

    @staticmethod
    def _spy(name, events):
        real = getattr(torch, name)

        def spy(*args, **kwargs):
            events.append(_describe("torch." + name, args, kwargs))
            return real(*args, **kwargs)
        return spy

    def __getattr__(self, name):
        return getattr(torch, name)


def issued(step, monkeypatch):
    """What the second call of step() issues (whatever is set up on a first call is not part of the sequence)."""
    step()
    events = []
    real_call, real_check = _lib.call, _lib.check

    def call_spy(name, *args):
        events.append("call " + name)
        return real_call(name, *args)

    def check_spy(code, what):
        events.append("check " + what)
        return real_check(code, what)

    def wrapper_spy(name):
        real = getattr(dense, name)

        def spy(*args, **kwargs):
            what = [a for a in args if isinstance(a, int)] if name == "weight_workspace" else \
                [tuple(job[:3]) for job in args[0]] if name == "reduce" else None
            events.append(_describe("dense." + name, args, kwargs) + ("" if what is None else " %s" % (what,)))
            return real(*args, **kwargs)
        return spy
    with monkeypatch.context() as m:
        m.setattr(_lib, "call", call_spy)
        m.setattr(_lib, "check", check_spy)
        for name in ("forward", "backward_input", "backward_pair", "backward_weight_partials", "gemm", "reduce", "weight_workspace"):
            m.setattr(dense, name, wrapper_spy(name))
        m.setattr(products, "torch", _TorchAsSeen(events))
        step()
    return events


def _step_of(mode, b, cin, c, mesh, gpu):
    nv, adj, csr = mesh
    torch.manual_seed(17)
    depth = 1 if mode in ("plain", "late") else 3
    stack = [layers.Batch_Image_ZERON_GCNGCN(cin, c).to(gpu) for _ in range(depth)]
    if mode == "batched":      # a layer of its own in front: the three equal ones then all read their input from the stacked buffers
        stack.insert(0, layers.Batch_Image_ZERON_GCNGCN(99, cin).to(gpu))
    x = torch.randn(b, nv, stack[0].in_features, device=gpu, requires_grad=True)
    seed = torch.randn(b, nv, c, device=gpu)

    def forward_backward(context):
        for p in [x] + [p for layer in stack for p in layer.parameters()]:
            p.grad = None
        with context:
            if mode == "stack":
                out = layers.zero_n_stack(x, csr, stack, F.relu)
            else:
                out = x
                for layer in stack:
                    out = layer(out, csr, F.relu)
            if mode != "batched":
                out.backward(seed)
        if mode == "batched":
            out.backward(seed)
        torch.cuda.synchronize()

    def step():
        if mode == "late":
            with layers.deferred_parameter_gradients():
                forward_backward(layers.late_input_gradients())
        elif mode == "batched":
            forward_backward(layers.weight_gradient_batching(depth=4))
        else:
            forward_backward(torch.enable_grad())
    return step, x, stack


def _issued_by(case, own, mesh, gpu, monkeypatch):
    name, mode, b, cin, c = case
    step, x, stack = _step_of(mode, b, cin, c, mesh, gpu)
    keep_own, keep_force = products.own_dense_products, fused.force
    products.own_dense_products = own
    if mode == "stack":
        fused.force = {"fwd": True, "bwd": True}
    try:
        events = issued(step, monkeypatch)
    finally:
        products.own_dense_products, fused.force = keep_own, keep_force
    assert x.grad is not None and all(p.grad is not None for layer in stack for p in layer.parameters())
    log = os.environ.get("GEOM_ROUTE_LOG")
    if log:
        with open(log, "a") as f:
            f.write("%s %s%s\n    %s\n" % (name, mode, " own" if own else "", "\n    ".join(events)))
    return events


# What the code issued before products.route() decided (recorded with GEOM_ROUTE_LOG from the three autograd nodes it replaced),
# keyed by (case, mode, own products preferred).  One deliberate difference, marked (b): inside weight_gradient_batching() the
# input gradient follows the preference for own products like everywhere else; each marked launch was `torch.matmul 4x162x48
# 48x48` (`48x99` for the first layer) there, the library's product whatever the preference said.
ROUTES = {
    ('648x48->48', 'plain', False): """
        torch.matmul 4x162x48 48x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 48, 48]
        dense.backward_pair 648x48 648x48 48x48 648x48 1500768
        call geom_dense_bwd_f32
        check geom_dense_bwd_f32
        dense.reduce [(648, 48, 48)]
        check geom_dense_reduce_f32
    """,
    ('648x48->48', 'plain', True): """
        dense.forward 648x48 48x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 48, 48]
        dense.backward_pair 648x48 648x48 48x48 648x48 1500768
        call geom_dense_bwd_f32
        check geom_dense_bwd_f32
        dense.reduce [(648, 48, 48)]
        check geom_dense_reduce_f32
    """,
    ('648x48->48', 'late', False): """
        torch.matmul 4x162x48 48x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 48, 48]
        dense.backward_pair 648x48 648x48 48x48 648x48 1500768
        call geom_dense_bwd_f32
        check geom_dense_bwd_f32
        check geom_dense_reduce2_f32
    """,
    ('648x48->48', 'late', True): """
        dense.forward 648x48 48x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 48, 48]
        dense.backward_pair 648x48 648x48 48x48 648x48 1500768
        call geom_dense_bwd_f32
        check geom_dense_bwd_f32
        check geom_dense_reduce2_f32
    """,
    ('648x99->48', 'plain', False): """
        torch.matmul 4x162x99 99x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 99, 48]
        torch.matmul 648x48 48x99
        dense.backward_weight_partials 648x99 648x48 2364528
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        dense.reduce [(648, 99, 48)]
        check geom_dense_reduce_f32
    """,
    ('648x99->48', 'plain', True): """
        dense.forward 648x99 99x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 99, 48]
        dense.backward_input 648x48 99x48
        call geom_dense_bwd_input_f32
        check geom_dense_bwd_input_f32
        dense.backward_weight_partials 648x99 648x48 2364528
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        dense.reduce [(648, 99, 48)]
        check geom_dense_reduce_f32
    """,
    ('648x99->48', 'late', False): """
        torch.matmul 4x162x99 99x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 99, 48]
        dense.backward_weight_partials 648x99 648x48 2364528
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        check geom_dense_reduce2_f32
        torch.mm 648x48 48x99 out=648x99
    """,
    ('648x99->48', 'late', True): """
        dense.forward 648x99 99x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 99, 48]
        dense.backward_weight_partials 648x99 648x48 2364528
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        check geom_dense_reduce2_f32
        dense.backward_input 648x48 99x48 out=648x99
        call geom_dense_bwd_input_f32
        check geom_dense_bwd_input_f32
    """,
    ('648x196->48', 'plain', False): """
        torch.matmul 4x162x196 196x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 196, 48]
        torch.matmul 648x48 48x196
        dense.backward_weight_partials 648x196 648x48 4724256
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        dense.reduce [(648, 196, 48)]
        check geom_dense_reduce_f32
    """,
    ('648x196->48', 'plain', True): """
        dense.forward 648x196 196x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 196, 48]
        dense.backward_input 648x48 196x48
        call geom_dense_bwd_input_f32
        check geom_dense_bwd_input_f32
        dense.backward_weight_partials 648x196 648x48 4724256
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        dense.reduce [(648, 196, 48)]
        check geom_dense_reduce_f32
    """,
    ('648x196->48', 'late', False): """
        torch.matmul 4x162x196 196x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 196, 48]
        dense.backward_weight_partials 648x196 648x48 4724256
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        check geom_dense_reduce2_f32
        torch.mm 648x48 48x196 out=648x196
    """,
    ('648x196->48', 'late', True): """
        dense.forward 648x196 196x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 196, 48]
        dense.backward_weight_partials 648x196 648x48 4724256
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        check geom_dense_reduce2_f32
        dense.backward_input 648x48 196x48 out=648x196
        call geom_dense_bwd_input_f32
        check geom_dense_bwd_input_f32
    """,
    ('648x40->40', 'plain', False): """
        dense.gemm 648x40 40x40
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x40 40x40 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x40 648x40 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
    """,
    ('648x40->40', 'plain', True): """
        dense.gemm 648x40 40x40
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x40 40x40 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x40 648x40 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
    """,
    ('648x40->40', 'late', False): """
        dense.gemm 648x40 40x40
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x40 40x40 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x40 648x40 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
    ('648x40->40', 'late', True): """
        dense.gemm 648x40 40x40
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x40 40x40 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x40 648x40 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
    ('324x48->48', 'plain', False): """
        dense.gemm 324x48 48x48
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 324x48 48x48 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 324x48 324x48 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
    """,
    ('324x48->48', 'plain', True): """
        dense.gemm 324x48 48x48
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 324x48 48x48 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 324x48 324x48 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
    """,
    ('324x48->48', 'late', False): """
        dense.gemm 324x48 48x48
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 324x48 48x48 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 324x48 324x48 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
    ('324x48->48', 'late', True): """
        dense.gemm 324x48 48x48
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 324x48 48x48 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 324x48 324x48 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
    ('648x48->16', 'plain', False): """
        dense.gemm 648x48 48x16
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x16 48x16 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x48 648x16 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
    """,
    ('648x48->16', 'plain', True): """
        dense.gemm 648x48 48x16
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x16 48x16 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x48 648x16 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
    """,
    ('648x48->16', 'late', False): """
        dense.gemm 648x48 48x16
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x16 48x16 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x48 648x16 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
    ('648x48->16', 'late', True): """
        dense.gemm 648x48 48x16
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x16 48x16 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x48 648x16 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
    ('162x48->48', 'plain', False): """
        torch.matmul 1x162x48 48x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
    """,
    ('162x48->48', 'plain', True): """
        torch.matmul 1x162x48 48x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
    """,
    ('162x48->48', 'late', False): """
        torch.matmul 1x162x48 48x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        check geom_colsum_batch_f32
    """,
    ('162x48->48', 'late', True): """
        torch.matmul 1x162x48 48x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        check geom_colsum_batch_f32
    """,
    ('648x192->3', 'plain', False): """
        dense.gemm 648x192 192x3
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x3 192x3 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x192 648x3 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
    """,
    ('648x192->3', 'plain', True): """
        dense.gemm 648x192 192x3
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x3 192x3 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x192 648x3 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
    """,
    ('648x192->3', 'late', False): """
        dense.gemm 648x192 192x3
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x3 192x3 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x192 648x3 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
    ('648x192->3', 'late', True): """
        dense.gemm 648x192 192x3
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.gemm 648x3 192x3 trans_b=True
        call geom_gemm_f32
        check geom_gemm_f32
        dense.gemm 648x192 648x3 trans_a=True
        call geom_gemm_f32
        check geom_gemm_f32
        check geom_colsum_batch_f32
    """,
    ('648x99->48 + 3x(648x48->48)', 'batched', False): """
        torch.matmul 4x162x99 99x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        torch.matmul 4x162x48 48x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        torch.matmul 4x162x48 48x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        torch.matmul 4x162x48 48x48
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        torch.matmul 4x162x48 48x48
        check geom_zn_gcn_aggregate_ell_bwd_f32
        torch.matmul 4x162x48 48x48
        check geom_zn_gcn_aggregate_ell_bwd_f32
        torch.matmul 4x162x48 48x48
        check geom_zn_gcn_aggregate_ell_bwd_f32
        torch.matmul 4x162x48 48x99
        check geom_colsum_batch_f32
        torch.mm 99x648 648x48 out=99x48
        torch.bmm 3x48x648 3x648x48 out=3x48x48
    """,
    ('648x99->48 + 3x(648x48->48)', 'batched', True): """
        dense.forward 648x99 99x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        dense.forward 648x48 48x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        dense.forward 648x48 48x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        dense.forward 648x48 48x48
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        (b) dense.backward_input 648x48 48x48
        (b) call geom_dense_bwd_input_f32
        (b) check geom_dense_bwd_input_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        (b) dense.backward_input 648x48 48x48
        (b) call geom_dense_bwd_input_f32
        (b) check geom_dense_bwd_input_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        (b) dense.backward_input 648x48 48x48
        (b) call geom_dense_bwd_input_f32
        (b) check geom_dense_bwd_input_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        (b) dense.backward_input 648x48 99x48
        (b) call geom_dense_bwd_input_f32
        (b) check geom_dense_bwd_input_f32
        check geom_colsum_batch_f32
        torch.mm 99x648 648x48 out=99x48
        torch.bmm 3x48x648 3x648x48 out=3x48x48
    """,
    ('3x(648x192->192)', 'stack', False): """
        torch.matmul 4x162x192 192x192
        call geom_zn_layer_fwd_f32
        check geom_zn_layer_fwd_f32
        call geom_zn_layer_fwd_f32
        check geom_zn_layer_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 192, 192]
        dense.backward_pair 648x192 648x192 192x192 648x192 2371584
        call geom_dense_bwd_f32
        check geom_dense_bwd_f32
        dense.reduce [(648, 192, 192)]
        check geom_dense_reduce_f32
        call geom_zn_layer_bwd_f32
        check geom_zn_layer_bwd_f32
        check geom_colsum_batch_f32
        dense.weight_workspace [648, 192, 192]
        dense.backward_weight_partials 648x192 648x192 2371584
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        dense.reduce [(648, 192, 192)]
        check geom_dense_reduce_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 192, 192]
        dense.backward_pair 648x192 648x192 192x192 648x192 2371584
        call geom_dense_bwd_f32
        check geom_dense_bwd_f32
        dense.reduce [(648, 192, 192)]
        check geom_dense_reduce_f32
    """,
    ('3x(648x192->192)', 'stack', True): """
        dense.forward 648x192 192x192
        call geom_dense_fwd_f32
        check geom_dense_fwd_f32
        call geom_zn_layer_fwd_f32
        check geom_zn_layer_fwd_f32
        call geom_zn_layer_fwd_f32
        check geom_zn_layer_fwd_f32
        check geom_zn_gcn_aggregate_ell_fwd_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 192, 192]
        dense.backward_pair 648x192 648x192 192x192 648x192 2371584
        call geom_dense_bwd_f32
        check geom_dense_bwd_f32
        dense.reduce [(648, 192, 192)]
        check geom_dense_reduce_f32
        call geom_zn_layer_bwd_f32
        check geom_zn_layer_bwd_f32
        check geom_colsum_batch_f32
        dense.weight_workspace [648, 192, 192]
        dense.backward_weight_partials 648x192 648x192 2371584
        call geom_dense_bwd_weight_f32
        check geom_dense_bwd_weight_f32
        dense.reduce [(648, 192, 192)]
        check geom_dense_reduce_f32
        check geom_zn_gcn_aggregate_ell_bwd_f32
        dense.weight_workspace [648, 192, 192]
        dense.backward_pair 648x192 648x192 192x192 648x192 2371584
        call geom_dense_bwd_f32
        check geom_dense_bwd_f32
        dense.reduce [(648, 192, 192)]
        check geom_dense_reduce_f32
    """,
}


@pytest.mark.parametrize("own", [False, True], ids=["library", "own"])
@pytest.mark.parametrize("case", CASES, ids=["%s-%s" % case[:2] for case in CASES])
def test_a_forward_and_backward_issue_what_they_issued(gpu, mesh, monkeypatch, case, own):
    events = _issued_by(case, own, mesh, gpu, monkeypatch)
    assert events == [line.strip().replace("(b) ", "") for line in ROUTES[(case[0], case[1], own)].strip().split("\n")]


# ---- a product whose forward runs on a kernel of this package is differentiable ------------------------------------------
def _layer64(x, w, bias, adj, k, seed):
    """float64 on the host: the support gradient dS = [A^T . g[..., :k] | g[..., k:]] of out = [A . S[..., :k] | S[..., k:]] + bias,
    S = x @ w, for the cotangent `seed` -- what both gradients of the product are products of."""
    g = seed.double().cpu()
    ds = torch.cat((adj.double().cpu().t() @ g[..., :k], g[..., k:]), dim=-1)
    return x.detach().double().cpu().reshape(-1, x.shape[-1]), ds.reshape(-1, ds.shape[-1]), w.detach().double().cpu().reshape(w.shape[-2:])


def test_frozen_weight_with_own_products_keeps_the_input_gradient(gpu, mesh):
    nv, adj, csr = mesh
    torch.manual_seed(5)
    layer = layers.Batch_Image_ZERON_GCNGCN(48, 48).to(gpu)
    layer.weight1.requires_grad_(False)
    x = torch.randn(4, nv, 48, device=gpu, requires_grad=True)
    seed = torch.randn(4, nv, 48, device=gpu)
    keep = products.own_dense_products
    products.own_dense_products = True
    try:
        out = layer(x, csr, None)
        out.backward(seed)
    finally:
        products.own_dense_products = keep
    assert x.grad is not None
    x64, ds64, w64 = _layer64(x, layer.weight1, layer.bias, adj, 16, seed)
    _rows_close(x.grad.view(-1, 48), ds64, w64.t(), "input gradient behind the package's own forward, frozen weight")


def test_own_forward_without_the_any_shape_kernel_keeps_both_gradients(gpu, mesh):
    nv, adj, csr = mesh
    torch.manual_seed(6)
    layer = layers.Batch_Image_ZERON_GCNGCN(48, 16).to(gpu)
    x = torch.randn(4, nv, 48, device=gpu, requires_grad=True)
    seed = torch.randn(4, nv, 16, device=gpu)
    keep = products.own_dense_products, products.use_any_shape_products
    products.own_dense_products, products.use_any_shape_products = True, False
    try:
        out = layer(x, csr, None)
        out.backward(seed)
    finally:
        products.own_dense_products, products.use_any_shape_products = keep
    assert x.grad is not None and layer.weight1.grad is not None
    x64, ds64, w64 = _layer64(x, layer.weight1, layer.bias, adj, 5, seed)
    _rows_close(x.grad.view(-1, 48), ds64, w64.t(), "input gradient behind the package's own forward, 48 -> 16")
    _rows_close(layer.weight1.grad.view(48, 16), x64.t(), ds64, "weight gradient behind the package's own forward, 48 -> 16")
