"""The frozen batched mesh encoder on ONE launch per layer and direction (csrc/encoder_stack.hip), and the latent loss.

`models.BatchMeshEncoder` takes this route when its parameters are frozen (`encoder.requires_grad_(False)`: the training step
of GEOMetrics.py only needs the latent loss's gradient with respect to the vertex positions).  A 0N-GCN layer aggregates its
first C // 10 columns only -- at most 30 here -- so the tail of layer l (gather + bias + ELU) is the operand load of layer
l + 1's product: 17 launches forward (the product of `h1`, sixteen layer boundaries), the existing aggregation for the head's
un-activated values, the segmented max over the vertices; backward the max's scatter and 17 mirrored launches that end in the
positions' gradient.  No weight product, no split-K reduction, no column sum is computed for parameters nobody trains.
"""
import os

import torch

from . import _lib
from . import aggregation as _agg

# The route of models.BatchMeshEncoder with frozen parameters: True = the launches of this module, False = the separate
# operators (one product + one aggregation per layer).  Opt-in (GEOM_ENCODER_FUSED=1) until tools/time_latent_loss.py has shown
# it faster than the separate operators on the same machine: profiles/latent_loss.txt.
enabled = os.environ.get("GEOM_ENCODER_FUSED", "0") == "1"

MAX_AGGREGATED = 32      # the aggregated columns must lie inside the product's first k-stage (geom_encoder_layer_*)


def serves(encoder, positions, adj):
    """Whether `encoder(positions, adj)` takes the fused route: the switch is on, fp32 [B,V,3] positions on the device, ONE
    adjacency (a dense [V,V] tensor or a CSR) and no parameter that requires grad."""
    from .layers import _Csr
    if not enabled or not torch.is_tensor(positions) or not positions.is_cuda:
        return False
    if positions.dtype != torch.float32 or positions.dim() != 3 or positions.shape[-1] != 3:
        return False
    if not (isinstance(adj, _Csr) or (torch.is_tensor(adj) and adj.dim() == 2 and adj.is_cuda)):
        return False
    if encoder.reduce.print_length // encoder.reduce.split > MAX_AGGREGATED:
        return False
    return not any(p.requires_grad for p in encoder.parameters())


def layer_forward(s, csr, k, bias, act, w, b, nv, x_out=None):
    """T(s) . w for s [b * nv, c] and w [c, n] (see include/geom_hip.h); x_out: receives T(s)."""
    c, n = w.shape
    out = torch.empty(b * nv, n, dtype=torch.float32, device=s.device)
    _lib.call("geom_encoder_layer_fwd_f32", b, nv, c, k, n, csr.rowptr, csr.col, csr.val, s, c, bias, act, w, n, out, n, x_out,
              c)
    return out


def layer_backward(g, x_saved, csr, k, act, w, b, nv, t_out=None):
    """T(g, x_saved) . w^T for g [b * nv, c] and w [n, c] (see include/geom_hip.h); t_out: receives T."""
    n, c = w.shape
    out = torch.empty(b * nv, n, dtype=torch.float32, device=g.device)
    _lib.call("geom_encoder_layer_bwd_f32", b, nv, c, k, n, csr.rowptr_t, csr.col_t, csr.val_t, g, c, x_saved, c, act, w, c,
              out, n, t_out, c)
    return out


class _FrozenTrunk(torch.autograd.Function):
    """positions [B,V,3] -> the head's un-activated values v [B,V,latent] (what BatchGCNMax takes the max of), through the
    sixteen ELU layers: one autograd node; params = (weight, bias) of every layer in order, the head's last."""

    @staticmethod
    def forward(ctx, positions, csr, want_grad, *params):
        pos = _lib.require(positions, "positions", torch.float32, 3, 3)
        b, nv, _ = pos.shape
        if nv != csr.nv:
            raise RuntimeError("positions have %d vertices but the adjacency has %d" % (nv, csr.nv))
        weights = [_lib.require(w, "weight", torch.float32, 2) for w in params[0::2]]
        biases = [_lib.require(t, "bias", torch.float32, 1) for t in params[1::2]]
        width = 3
        for w, bias in zip(weights, biases):
            if w.shape[0] != width or bias.shape[0] != w.shape[1]:
                raise RuntimeError("encoder layer shapes do not chain: weight %s after width %d" % (tuple(w.shape), width))
            width = w.shape[1]
        s = layer_forward(pos.view(b * nv, 3), csr, 0, None, _agg.ACT_NONE, weights[0], b, nv)
        saved = []
        for w, bias, w_next in zip(weights[:-1], biases[:-1], weights[1:]):
            c = w.shape[1]
            x = torch.empty(b * nv, c, dtype=torch.float32, device=pos.device) if want_grad else None
            s = layer_forward(s, csr, c // 10, bias, _agg.ACT_ELU, w_next, b, nv, x_out=x)
            saved.append(x)
        latent = weights[-1].shape[1]
        v = torch.empty(b, nv, latent, dtype=torch.float32, device=pos.device)
        _agg.forward(s.view(b, nv, latent), biases[-1], csr, latent // 10, _agg.ACT_NONE, v)
        ctx.csr, ctx.shape = csr, (b, nv)
        if want_grad:
            ctx.save_for_backward(*weights, *saved)
        ctx.layers = len(weights)
        return v

    @staticmethod
    def backward(ctx, grad_v):
        b, nv = ctx.shape
        weights, saved = ctx.saved_tensors[:ctx.layers], ctx.saved_tensors[ctx.layers:]
        g = grad_v.contiguous().view(b * nv, -1)
        # the head: no activation in front of its max; then the sixteen ELU layers, last to first
        g = layer_backward(g, None, ctx.csr, g.shape[1] // 10, _agg.ACT_NONE, weights[-1], b, nv)
        for w, x in zip(reversed(weights[:-1]), reversed(saved)):
            g = layer_backward(g, x, ctx.csr, w.shape[1] // 10, _agg.ACT_ELU, w, b, nv)
        return (g.view(b, nv, 3), None, None) + (None,) * (2 * ctx.layers)


def pre_max(encoder, positions, csr):
    """The fused route up to the values the head takes its max of, [B,V,latent]."""
    params = []
    for name, _, _ in encoder._WIDTHS:
        layer = getattr(encoder, name)
        params += [layer.weight, layer.bias]
    params += [encoder.reduce.weight_Ws[0], encoder.reduce.weight_Bs[0]]
    want_grad = torch.is_grad_enabled() and positions.requires_grad
    return _FrozenTrunk.apply(positions, csr, want_grad, *params)


def vertex_max(v):
    """max over the vertices of v [B,V,C] -> [B,C] on the segmented-max kernels (uniform segments; the arg-max is kept for the
    backward, lowest vertex on ties)."""
    from .ops import SegmentMax
    b, nv, c = v.shape
    offsets = torch.arange(0, (b + 1) * nv, max(nv, 1), dtype=torch.int64, device=v.device)[:b + 1]
    return SegmentMax.apply(v.reshape(b * nv, c), offsets, nv)


class _LatentL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, on, weight):
        p = _lib.require(pred, "latent_pred", torch.float32, 2)
        t = _lib.require(target, "train_latent", torch.float32, 2)
        o = _lib.require(on, "on_latent", torch.float32, 1)
        _lib.same_device(p, t, o)
        if t.shape != p.shape or o.shape[0] != p.shape[0]:
            raise RuntimeError("latent_loss: latent_pred %s, train_latent %s and on_latent %s do not match"
                               % (tuple(p.shape), tuple(t.shape), tuple(o.shape)))
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        _lib.call("geom_latent_l1_fwd_f32", p.shape[0], p.shape[1], p, t, o, float(weight), loss)
        ctx.save_for_backward(p, t, o)
        ctx.weight = float(weight)
        return loss.view(())

    @staticmethod
    def backward(ctx, grad_loss):
        p, t, o = ctx.saved_tensors
        go = grad_loss.contiguous().view(1)
        grad = torch.empty_like(p)
        _lib.call("geom_latent_l1_bwd_f32", p.shape[0], p.shape[1], p, t, o, ctx.weight, go, grad)
        return grad, None, None, None


def latent_loss(latent_pred, train_latent, on_latent, weight=.0005):
    """weight * sum_b [ mean_j |latent_pred - train_latent| * on_latent / sum(on_latent) ] (GEOMetrics.py:167) as one autograd
    node on two kernels, differentiable in latent_pred.  Where the reference asks the host whether any mesh of the batch has
    a latent (`on_latent.sum() != 0`, line 165) the kernels decide: no such mesh gives 0 and a zero gradient, with no host
    read -- the step stays capturable."""
    on = on_latent if on_latent.dtype == torch.float32 else on_latent.to(torch.float32)
    return _LatentL1.apply(latent_pred, train_latent, on.reshape(-1), weight)
