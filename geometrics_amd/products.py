"""The dense product `support = input @ W` at the head of every 0N-GCN layer, and its two gradients: which kernel computes each
(`route`: one rule of plain values), the one autograd node that runs them (`_Product`), the backward bodies it shares with the
fused layer boundary (`product_gradients`), and the stacked buffers that let a run of equal layers compute its weight gradients
as one batched product (`weight_gradient_batching`).  geometrics_amd.layers calls `_dense(x, w)`.
"""
import os
import threading
from collections import namedtuple

import torch

from . import backward_pass as _pass
from . import dense as _dense_kernels
from . import gemm_tuning


# ---- weight gradients of a stack of equal layers as ONE batched product --------------------------------------------------
# dW = X^T . G of a hidden layer (K = b*V rows against a 192 x 192 output) is the library's least efficient product: 22 us at
# the reference's training shape for 0.57 GFLOP, and a deformation block issues twelve of them, one per layer.  The
# gradients are independent of each other, so inside `weight_gradient_batching()` they are postponed to the end of the
# backward pass (geometrics_amd.backward_pass: same mechanism and safeguards as the bias gradients) and issued as one
# strided-batched product per run of equal layers: 242 -> 72 us for the twelve.  A strided-batched product wants its operands
# at a regular pitch, so while the context is active the layers' activations and gradients are carved out of stacked buffers
# (`_Slabs`): consecutive equal-shape allocations sit one pitch apart, forward ones ascending, backward ones descending
# (the backward pass meets the layers in reverse), which makes X_l, G_l and dW_l all ascending in l.
class _Slabs:
    """Stacked buffers for the tensors of one forward/backward pass: take(kind, shape) returns the next [shape] slot of a
    [slots, *shape] buffer of that kind and shape (a fresh buffer when the current one is used up: the run of equal
    layers is then split there).  slots = the depth of the stack (untaken slots cost address space only)."""
    def __init__(self, slots):
        self.open = {}
        self.slots = max(2, int(slots))

    def take(self, kind, shape, device, descending=False):
        shape = tuple(shape)
        key = (kind, shape, device, descending)
        slots = self.slots
        cur = self.open.get(key)
        if cur is None or cur[1] == slots:
            cur = self.open[key] = [torch.empty((slots,) + shape, dtype=torch.float32, device=device), 0]
        index = slots - 1 - cur[1] if descending else cur[1]
        cur[1] += 1
        return cur[0][index]


_active = threading.local()    # .slabs = the arena of the forward pass running on this thread (weight_gradient_batching)


def current_slabs():
    return getattr(_active, "slabs", None)


class weight_gradient_batching:
    """Context manager for the FORWARD pass of a stack of layers: their weight gradients are computed at the end of the
    backward pass, batched over runs of equal layers (see above).  Results differ from the per-layer products only by the
    library kernel's summation order (1e-6 relative)."""

    def __init__(self, depth=4):
        """depth: how many equal layers follow each other at most (the slots of one stacked buffer)."""
        self.depth = depth

    def __enter__(self):
        self.outer = current_slabs()
        # nothing to batch without a backward pass: an inference forward keeps its plain, progressively freed allocations
        _active.slabs = _Slabs(self.depth) if torch.is_grad_enabled() else None
        return self

    def __exit__(self, *exc):
        _active.slabs = self.outer
        return False


def _new_like(t, kind, arena, descending=False):
    """Allocation of an activation / gradient: a slot of the pass's stacked buffers when batching is on."""
    if arena is None:
        return torch.empty_like(t)
    return arena.take(kind, t.shape, t.device, descending)


def _regular_run(tensors):
    """(first tensor, pitch in elements) when the tensors sit at one constant positive pitch inside one storage."""
    first = tensors[0]
    if len(tensors) == 1:
        return first, 0
    base = first.untyped_storage().data_ptr()
    if any(t.untyped_storage().data_ptr() != base or t.stride() != first.stride() for t in tensors):
        return None
    step = tensors[1].storage_offset() - first.storage_offset()
    if step <= 0 or any(tensors[i + 1].storage_offset() - tensors[i].storage_offset() != step for i in range(len(tensors) - 1)):
        return None
    return first, step


def _launch_weight_products(jobs):
    """A pass's postponed weight-gradient products in layer order: batched over runs of equal layers at a regular pitch."""
    i = 0
    while i < len(jobs):
        first = jobs[i]
        j = i + 1
        while (j < len(jobs) and jobs[j].x.shape == first.x.shape and jobs[j].g.shape == first.g.shape
               and jobs[j].stream == first.stream):
            j += 1
        group = jobs[i:j]
        with torch.cuda.stream(first.stream), torch.no_grad():
            runs = [_regular_run([getattr(job, name) for job in group]) for name in ("x", "g", "out")] if len(group) > 1 else None
            if runs and all(runs):
                xb, gb, ob = (torch.as_strided(run[0], (len(group),) + tuple(t.shape), (run[1],) + tuple(t.stride()))
                              for run, t in zip(runs, (first.x, first.g, first.out)))
                torch.bmm(xb.transpose(1, 2), gb, out=ob)
            else:
                for job in group:
                    # (a layer of its own width -- the block's 192 -> 3 coordinate head: 7712 summed rows against a 192 x 3 output
                    # is 75 us in the library, which runs it without a split; the any-shape kernel splits the sum)
                    dw = route(job.x.shape[0], job.x.shape[1], job.g.shape[1], True, True, True, True, False, use_any_shape_products).dw
                    _weight_product(dw, job.x, job.g, out=job.out)
        i = j


# ---- which kernel computes a product ------------------------------------------------------------------------------------
use_any_shape_products = True         # the widths the 192-column kernels do not take: csrc/dense_any.hip (False: the library's products)

# The library's products of this path are fast only with the recorded selections of geometrics_amd/tuning (TunableOp: validated
# against the PyTorch / hipBLASLt build, so a library update REJECTS the file and the default heuristic runs the 963-wide
# products at 85 us instead of 62).  When gemm_tuning.enable() was called and the file was rejected, the forward products and
# the wide input gradient of the 192-column layers take this package's own matrix-core kernels instead (csrc/dense_gemm.hip:
# within a few per cent of the tuned library, measured by tools/time_dense.py and, in a whole step, by bench.py run with
# GEOM_OWN_PRODUCTS=1): the headline does not hang on a version-locked file.  None = that rule; True / False force it (tests, A/B).
own_dense_products = None


def _own_products_preferred():
    if own_dense_products is not None:
        return bool(own_dense_products)
    env = os.environ.get("GEOM_OWN_PRODUCTS")
    if env is not None:
        return env not in ("", "0")
    return gemm_tuning.status == "library default (tuning file rejected)"      # (not: "tuned at start-up", gemm_tuning.tune_products)


# forward: "any" (dense.gemm) | "own" (dense.forward) | "lib";  dx: "pair" (one launch with the weight partials) | "any" | "own"
# (dense.backward_input) | "lib";  dw: "split" (partial sums + the end-of-pass reduction) | "any" | "lib";  node: the product needs
# _Product (False: all three are the library's, and torch.matmul under torch's own autograd computes exactly them)
Route = namedtuple("Route", "forward dx dw node")


def route(rows, cin, c, w_requires_grad, w_contiguous, x_contiguous, batched, own, any_allowed):
    """THE rule: which kernel runs x [rows, cin] @ w [cin, c] and each of its gradients, for fp32 operands on the device.
    w_requires_grad / w_contiguous: of the weight;  x_contiguous: of x as [rows, cin];  batched: the forward runs inside
    weight_gradient_batching() (the weight gradient is then postponed to the pass's batched product where it may be: `dw` is
    the kernel that computes it when it may not);  own: _own_products_preferred();  any_allowed: use_any_shape_products."""
    plan = _dense_kernels.plan(rows, cin, c)
    split = plan["dw"] == "mfma"
    # the any-shape kernel (csrc/dense_any.hip): whatever the 192-column kernels (dense.plan) do not take -- the mesh encoder's
    # 3 / 60 / ... / 300-wide ZERON_GCN layers, whose weight gradients (18 432 summed rows against a 300 x 300 output) the library
    # runs without a split, 73-97 us each
    any_shape = any_allowed and not split and _dense_kernels.any_supported(rows, cin, c)
    lib_or_own = "own" if (own and w_contiguous and c % 16 == 0 and rows >= 512 and _dense_kernels.supported(cin, c, rows)) else "lib"
    forward = "any" if any_shape and w_contiguous else lib_or_own
    if batched:
        return Route(forward, lib_or_own, "any" if any_shape else "lib", True)
    if split and w_requires_grad:
        if x_contiguous and w_contiguous:
            return Route(forward, "pair" if plan["pair"] else lib_or_own, "split", True)
        return Route(forward, lib_or_own, "lib", lib_or_own == "own")
    if forward == "any":
        return Route("any", "any", "any", True)
    return Route(forward, lib_or_own, "lib", lib_or_own == "own")


def _input_gradient(kind, g, w2, out=None):
    """g @ w2^T (g [.., c], w2 [cin, c]) on the kernel `kind` names; g and w2 contiguous for "any" / "own"."""
    if kind == "any":
        return _dense_kernels.gemm(g, w2, trans_b=True, out=out)
    if kind == "own":
        return _dense_kernels.backward_input(g, w2, out=out)
    # "lib": the library's product -- or, where dense.wide_dx_plan says so (the 963-wide first layer at training size), the
    # same product on the bf16 matrix cores.  route() does not know the difference: the kind names who owns the product's
    # values (exact fp32 products, an fp32 sum), not which launch computes them
    if _dense_kernels.wide_dx_takes(g, w2, out):
        dx = _dense_kernels.backward_input_split(g.view(-1, g.shape[-1]), w2, out=out)
        return dx if out is not None else dx.view(g.shape[:-1] + (w2.shape[0],))
    return torch.matmul(g, w2.t()) if out is None else torch.mm(g, w2.t(), out=out)


def _weight_product(kind, x2, g2, out=None):
    """x2^T @ g2 ([rows, cin]^T x [rows, c]): the any-shape kernel's split product for "any", given rows of unit stride (the
    library runs a long sum against a small output without a split: 75 us for the 192 -> 3 head at 7712 rows), else the library."""
    if kind == "any" and x2.stride(1) == 1 and g2.stride(1) == 1 and (out is None or (out.dim() == 2 and out.stride(1) == 1)):
        return _dense_kernels.gemm(x2, g2, trans_a=True, out=out)
    return torch.mm(x2.t(), g2) if out is None else torch.mm(x2.t(), g2, out=out)


def product_gradients(x, g, w, w_ref, route, need_x, need_w, arena=None, dx=None, leaf=None):
    """(dX shaped like x, dW shaped like w) of x @ w for the gradient g of the product (contiguous), by the kernels `route`
    names; None for a gradient that is not needed.  w_ref: the weak reference of _pass.parameter_ref.  arena: the stacked
    buffers of weight_gradient_batching() the forward ran in.  dx: dX when somebody computed it already (a fused boundary's
    launch).  leaf: x itself when dX may be postponed to the end of the pass (_pass.may_postpone_input_gradient)."""
    w2 = w.reshape(w.shape[-2:])
    cin, c = w2.shape
    x2, g2 = x.reshape(-1, cin), g.view(-1, c)
    rows = g2.shape[0]
    need_x = need_x and dx is None
    if route.dw == "split" and need_w:
        # the split partial sums of dW on the matrix cores -- with dX in the same launch (two workgroups per CU) for the 192-wide
        # layers, alone for the 963-wide one; the partials of all layers of a backward pass are added up by one reduction launch
        # at its end inside `deferred_parameter_gradients()`, at once otherwise.  Same values either way: the order is fixed.
        ws = _dense_kernels.weight_workspace(rows, cin, c, x.device)
        if need_x and route.dx == "pair":
            dx = torch.empty_like(x)
            _dense_kernels.backward_pair(x2, g2, w2, dx.view(rows, cin), ws)
        else:
            if need_x and leaf is not None and _pass.may_postpone_input_gradient(leaf):
                # no gradient for x through the engine: the end-of-pass callback launches the product behind the reduction
                # launch and makes its buffer the leaf's .grad
                late = torch.empty(rows, cin, dtype=x.dtype, device=x.device)
                _pass.postpone_input_gradient(lambda: _input_gradient(route.dx, g2, w2, out=late), late, leaf)
            elif need_x:
                dx = _input_gradient(route.dx, g2, w2).view(x.shape)
            _dense_kernels.backward_weight_partials(x2, g2, ws)
        return dx, _pass.weight_gradient(w_ref, w, rows, cin, c, ws)
    if need_x:
        # (inside weight_gradient_batching() the library gets the gradient in the product's own shape, as it always did)
        dx = _input_gradient(route.dx, g if arena is not None and route.dx == "lib" else g2, w2).view(x.shape)
    grad_w = None
    if need_w:
        param = w_ref() if arena is not None else None
        if param is not None and x2.is_contiguous() and _pass.may_defer(param, opted_in=True):
            grad_w = arena.take("dW", w.shape, w.device, descending=True)
            _pass.postpone_weight_product(x2, g2, grad_w, w_ref, _launch_weight_products)
        else:
            grad_w = _weight_product(route.dw, x2, g2).view(w.shape)
    return dx, grad_w


class _Product(torch.autograd.Function):
    """support = input @ W for [.., Cin] x [Cin, Cout] (W may carry the reference's leading 1: [1, Cin, Cout]) on the kernels
    `route` names.  Takes the PARAMETER itself, so that its gradient goes straight to the leaf."""

    @staticmethod
    def forward(ctx, x, w, route, arena):
        ctx.route, ctx.arena = route, arena
        ctx.w_ref = _pass.parameter_ref(w, ctx, ctx.needs_input_grad[1])
        x, out = _forward(route.forward, x, w.reshape(w.shape[-2:]))
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        dx, dw = product_gradients(x, grad.contiguous(), w, ctx.w_ref, ctx.route, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                   ctx.arena, leaf=x)
        return dx, dw, None, None


def _forward(kind, x, w2):
    """(x as the kernel read it, x @ w2).  x is made contiguous only when a kernel of ours takes it; the copy is then what the
    backward pass reads, too."""
    if kind == "lib":
        return x, torch.matmul(x, w2)
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
        x = x2.view(x.shape)
    out = _dense_kernels.gemm(x2, w2) if kind == "any" else _dense_kernels.forward(x2, w2)
    return x, out.view(x.shape[:-1] + (w2.shape[1],))


def _dense(x, w):
    """input @ weight of a 0N-GCN layer; w = the layer's weight parameter ([Cin, Cout] or [1, Cin, Cout])."""
    # what every kernel of ours asks of its operands; anything else is the library's product under torch's own autograd
    # ([1,Cin,Cout]: one GEMM, not B broadcast bmm's)
    if not (x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32
            and (w.dim() == 2 or (w.dim() == 3 and w.shape[0] == 1)) and x.shape[-1] == w.shape[-2]):
        return torch.matmul(x, w.squeeze(0) if w.dim() == 3 else w)
    differentiable = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)
    arena = current_slabs() if differentiable else None
    cin = x.shape[-1]
    r = route(x.numel() // max(cin, 1), cin, w.shape[-1], w.requires_grad, w.is_contiguous(),
              x.is_contiguous() or x.reshape(-1, cin).is_contiguous(), arena is not None, _own_products_preferred(),
              use_any_shape_products)
    if differentiable and r.node:
        return _Product.apply(x, w, r, arena)
    return _forward(r.forward, x, w.reshape(w.shape[-2:]))[1]      # (the same kernel as the node picks for the shape)
