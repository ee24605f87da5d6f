"""0N-GCN layers with the reference's class names, constructor signatures, parameter names
and initialisers (reference layers.py:14-189), so `models.py` and pretrained state_dicts
(`gcN.weight1`, `gcN.weight`, `gcN.bias`, `weight_Ws.0`, `weight_Bs.0`) work unchanged.

`forward(input, adj, activation)` still receives the DENSE [V,V] adjacency the callers pass
(models.py:241, GEOMetrics.py:120).  The layer derives CSR and CSR^T from it once (cached on
the tensor's identity + version) and replaces the reference's dense `adj @ support[..., :k]`,
`torch.cat` and bias add by one fused HIP kernel (csrc/zn_gcn.hip, launched by `aggregation.py`); which
kernel computes the feature product `input @ W` and its gradients is `products.route()`'s decision.
"""
import math
import os

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn import Module
from torch.nn.parameter import Parameter

from . import _lib
from . import aggregation as _agg
from . import backward_pass as _pass
from . import fused as _fused
from . import products as _products
from ._identity import ByTensor, MemoryStamp
# (re-exported: bench.py and dist.py use the public names, models, ops, deform and the tests the private ones)
from .backward_pass import (_alias, _gradient_buffer, bind_gradient_targets, deferred_parameter_gradients,  # noqa: F401
                            late_input_gradients)
# (the layers' dense products; the flags that steer them are set on geometrics_amd.products, not here)
from .products import _dense, _new_like, current_slabs, weight_gradient_batching  # noqa: F401
# (the aggregation's launches; tools and tests call the two launchers under these names)
from .aggregation import ACT_ELU as _ACT_ELU, ACT_NONE as _ACT_NONE, ACT_RELU as _ACT_RELU  # noqa: F401
from .aggregation import activation_code as _activation_code, backward as aggregate_backward, forward as aggregate_forward  # noqa: F401


# --------------------------------------------------------------- CSR cache ----
class _Csr:
    __slots__ = ("rowptr", "col", "val", "rowptr_t", "col_t", "val_t", "nv", "nnz",
                 "ell_w", "ell_col", "ell_val", "ell_col_t", "ell_val_t", "inv_deg", "over", "over_t",
                 "symmetric_structure",
                 "_deform_tail",      # (geometrics_amd.deform: the rows' entries beyond the table as a second fixed-width table)
                 "_deform_plain")     # (geometrics_amd.deform: 8-wide tables + CSR overflow lists of A and A^T, whatever ell_w is)


_csr_cache = ByTensor()   # adjacency tensor -> its _Csr


def _to_csr(dense):
    nz = dense.nonzero()                       # row-major order == CSR order
    rows, cols = nz[:, 0], nz[:, 1]
    counts = torch.bincount(rows, minlength=dense.shape[0])
    rowptr = torch.zeros(dense.shape[0] + 1, dtype=torch.int64, device=dense.device)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr.to(torch.int32), cols.to(torch.int32).contiguous(), dense[rows, cols].to(torch.float32).contiguous()


def _to_ell(rowptr, col, val, width):
    """[V][width] neighbour table holding the first `width` entries of every CSR row (unused slots col = -1 /
    val = 0) + the CSR tail (over_ptr, over_col, over_val) of the rows that are longer, or None when none is."""
    nv = rowptr.numel() - 1
    lens = (rowptr[1:] - rowptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(nv, device=col.device), lens)
    slot = torch.arange(col.numel(), device=col.device) - rowptr[:-1].long()[rows]
    ell_col = torch.full((nv, width), -1, dtype=torch.int32, device=col.device)
    ell_val = torch.zeros((nv, width), dtype=torch.float32, device=col.device)
    head = slot < width
    ell_col[rows[head], slot[head]] = col[head]
    ell_val[rows[head], slot[head]] = val[head]
    over = None
    if not bool(head.all()):
        over_ptr = torch.zeros(nv + 1, dtype=torch.int64, device=col.device)
        over_ptr[1:] = torch.cumsum((lens - width).clamp_min(0), 0)
        over = (over_ptr.to(torch.int32).contiguous(), col[~head].contiguous(), val[~head].contiguous())
    return ell_col.contiguous(), ell_val.contiguous(), over


def _ell_width(lens_a, lens_b):
    """Table width of the fast kernel: the smallest of 8 / 16 that leaves at most 5 % of the rows (of either
    orientation) with a CSR tail -- an icosphere (rows of 6-7) gets 8 and no tail, the reference's 482.obj (rows of
    5-9 and two poles of 33) gets 8 with a 10-row tail; 0 = irregular degrees, generic CSR kernel."""
    n = max(int(lens_a.numel()), 1)
    for w in (8, 16):
        if max(int((lens_a > w).sum()), int((lens_b > w).sum())) <= 0.05 * n:
            return w
    return 0


def _finish_csr(c):
    """Derived tables shared by every construction route: 1/(degree without the self loop) and, for bounded
    degrees, the fixed-stride ELL neighbour tables of the fast aggregation kernel."""
    c.nv = int(c.rowptr.numel()) - 1
    c.nnz = int(c.col.numel())
    # 1 / (neighbours without the self loop): what batch_get_lap_info divides by on the binary adjacency
    c.inv_deg = (1.0 / ((c.rowptr[1:] - c.rowptr[:-1]).float() - 1.0)).contiguous()
    c.ell_w = _ell_width(c.rowptr[1:] - c.rowptr[:-1], c.rowptr_t[1:] - c.rowptr_t[:-1]) if c.nv else 0
    # A[u][v] != 0 exactly where A[v][u] != 0 (values may differ): every route builds rows with their columns in ascending
    # order, so the pattern is symmetric iff CSR and CSR^T have the same (rowptr, col).  The chain launches of
    # geometrics_amd.deform rely on it (a vertex waits only on the vertices of its own row before it overwrites its row).
    c.symmetric_structure = bool(torch.equal(c.rowptr, c.rowptr_t) and torch.equal(c.col, c.col_t))
    c.ell_col = c.ell_val = c.ell_col_t = c.ell_val_t = c.over = c.over_t = None
    if c.ell_w:
        c.ell_col, c.ell_val, c.over = _to_ell(c.rowptr, c.col, c.val, c.ell_w)
        c.ell_col_t, c.ell_val_t, c.over_t = _to_ell(c.rowptr_t, c.col_t, c.val_t, c.ell_w)
    return c


def csr_from_parts(rowptr, col, val, rowptr_t, col_t, val_t, derive=True):
    """An adjacency handed over already in CSR (+ CSR^T): int32 rowptr/col, fp32 val, on the device.  The result
    can be passed wherever a layer takes `adj` (geometrics_amd.ragged builds block-diagonal batches this way).
    derive=False: the six arrays alone, nothing read on the host (utils.ragged_split_info inside a captured step); the
    derived tables (_finish_csr: the ELL width is a host decision) are made when adjacency_csr first sees the object, as
    for a CSR handed over through register_csr."""
    c = _Csr()
    c.rowptr, c.col, c.val, c.rowptr_t, c.col_t, c.val_t = rowptr, col, val, rowptr_t, col_t, val_t
    if not derive:
        return c
    with torch.no_grad():
        return _finish_csr(c)


def adjacency_csr(adj):
    """CSR + CSR^T (+ ELL tables) of a dense [V,V] adjacency, cached per TENSOR OBJECT and in-place
    version (_identity.ByTensor: never the data pointer, which the caching allocator hands to the next
    adjacency of the same size -- auto_encoder.py builds a fresh one per mesh).  Building reads the dense
    matrix once (one host sync, at first use only)."""
    if isinstance(adj, _Csr):
        if not hasattr(adj, "ell_w"):              # csr_from_parts(derive=False): its derived tables are made at first use
            with torch.no_grad():
                _finish_csr(adj)
        return adj
    if hasattr(adj, "csr") and isinstance(adj.csr, _Csr):     # a RaggedMeshBatch
        return adj.csr
    if adj.dim() != 2 or adj.shape[0] != adj.shape[1]:
        raise RuntimeError("adjacency must be a square [V,V] tensor, got %s" % (tuple(adj.shape),))
    hit = _csr_cache.get(adj)
    if hit is not None:
        if not hasattr(hit, "ell_w"):          # handed over by register_csr: its derived tables are made at first use
            with torch.no_grad():
                _finish_csr(hit)
        return hit
    if not adj.is_cuda:
        raise RuntimeError("adjacency must live on a HIP device; geometrics_amd has no CPU path")
    with torch.no_grad():
        c = _Csr()
        dense = adj.detach()
        c.rowptr, c.col, c.val = _to_csr(dense)
        c.rowptr_t, c.col_t, c.val_t = _to_csr(dense.t())
        _finish_csr(c)
    return _csr_cache.put(c, adj)


def register_csr(adj, csr):
    """Hand over the CSR (+ CSR^T) of the dense adjacency `adj` that its maker already has (utils.split_info fills the dense
    matrix FROM the CSR): adjacency_csr(adj) then returns this object instead of reading the matrix back through nonzero().
    csr: a _Csr (csr_from_parts), or the six arrays of csr_from_parts as a tuple -- registering those reads nothing on the
    host; the derived tables (_finish_csr: the ELL width is a host decision) are made when the object is first asked for.
    Same cache as adjacency_csr (_identity.ByTensor: tensor object + in-place version).  Returns the object."""
    if not isinstance(csr, _Csr):
        c = _Csr()
        c.rowptr, c.col, c.val, c.rowptr_t, c.col_t, c.val_t = csr
        csr = c
    return _csr_cache.put(csr, adj)


def registered_csr(adj):
    """The cached CSR of `adj` as it stands -- possibly without its derived tables (only rowptr / col / val and their
    transposes are promised) -- or None: for callers that need the pattern alone and must not read the host."""
    return _csr_cache.get(adj)


# ------------------------------------------------------- fused aggregation ----
def _route(activation, t, adj, any_input=False):
    """(activation, the tensor an entry below is given, adj) -> the kernel's activation code; `foreign`: a callable the kernels do
    not know, applied by the caller afterwards; `batched`: an fp32 [B,V,C] device tensor with ONE adjacency, what the head and the
    boundary launches take; the CSR, built for a batched input only unless `any_input` (zero_n_aggregate: everything but a dense
    adjacency per mesh, [B,V,V], which has none and takes the torch path)."""
    act = _ACT_NONE if activation is None else _activation_code(activation)
    per_mesh = torch.is_tensor(adj) and adj.dim() == 3
    batched = torch.is_tensor(t) and t.dim() == 3 and t.is_cuda and t.dtype == torch.float32 and not per_mesh
    csr = adjacency_csr(adj) if batched or (any_input and not per_mesh) else None
    return act, activation is not None and act == _ACT_NONE, batched, csr


def _split_k(support, layer):
    return support.shape[-1] // layer.split        # the leading columns of a layer's support that are aggregated


def _bias_for(ctx):
    """(a bias gradient is wanted, the bias parameter) of a node that kept `bias_ref` in its forward."""
    wanted = ctx.needs_input_grad[1] and ctx.bias_ref is not None
    return wanted, (ctx.bias_ref() if wanted else None)


class _ZeroNAggregate(torch.autograd.Function):
    """out = act([A . S[..., :k] | S[..., k:]] + bias)  for S [B,V,C]: one kernel, S read once.
    Backward: grad_S = [A^T . g[..., :k] | g[..., k:]] with g = grad_out * act'(out), again one kernel."""

    @staticmethod
    def forward(ctx, support, bias, csr, k, act):
        s = _lib.require(support, "support", torch.float32, 3)
        if s.shape[1] != csr.nv:
            raise RuntimeError("support has %d vertices but the adjacency has %d" % (s.shape[1], csr.nv))
        bias_c = None if bias is None else _lib.require(bias, "bias", torch.float32, 1)
        ctx.arena = current_slabs()
        out = _new_like(s, "aggregated", ctx.arena)
        mask = _agg.forward(s, bias_c, csr, k, act, out, want_mask=support.requires_grad)
        ctx.csr, ctx.k, ctx.act = csr, k, act
        ctx.bias_ref = _pass.parameter_ref(bias, ctx, ctx.needs_input_grad[1])
        ctx.masked = mask is not None
        if mask is not None:
            ctx.save_for_backward(mask)
        elif act != _ACT_NONE:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        mask = ctx.saved_tensors[0] if ctx.masked else None
        out = ctx.saved_tensors[0] if (ctx.act != _ACT_NONE and not ctx.masked) else None
        grad_support, grad_bias = _agg.backward(grad_out.contiguous(), ctx.csr, ctx.k, ctx.act, out, mask, *_bias_for(ctx),
                                                arena=ctx.arena)
        return (grad_support if ctx.needs_input_grad[0] else None), grad_bias, None, None, None


class _ZeroNAggregateHead(torch.autograd.Function):
    """positions = base + scale * act([A . S[..., :k] | S[..., k:]] + bias)[..., :3]: the aggregation of the layer whose
    three leading channels are a stage's coordinate update (GEOMetrics.py:121,126,131), with the update in the same two
    launches.  Forward: the aggregation kernel also writes the new positions.  Backward: the gradient of the layer output
    is [scale * grad_pos | 0 ...] by construction -- it is never materialised (15.7 MB of zeros at the BASELINE shard) nor
    read back; the aggregation backward synthesises it from grad_pos."""

    @staticmethod
    def forward(ctx, support, bias, base, csr, k, act, scale, down=None):
        s = _lib.require(support, "support", torch.float32, 3)
        base_c = _lib.require(base, "base", torch.float32, 3, 3)
        ctx.down = down        # a _StackLink: the boundary launch that produced `support` (zero_n_stack_positions)
        bias_c = None if bias is None else _lib.require(bias, "bias", torch.float32, 1)
        pos = torch.empty_like(base_c)
        mask = _agg.forward(s, bias_c, csr, k, act, torch.empty_like(s), want_mask=True, head=(base_c, scale, pos))
        ctx.csr, ctx.k, ctx.act, ctx.scale, ctx.shape = csr, k, act, float(scale), tuple(s.shape)
        ctx.bias_ref = _pass.parameter_ref(bias, ctx, ctx.needs_input_grad[1])
        if mask is not None:
            ctx.save_for_backward(mask)
        return pos

    @staticmethod
    def backward(ctx, grad_pos):
        gp = grad_pos.contiguous()
        b, nv, c = ctx.shape
        mask = ctx.saved_tensors[0] if ctx.saved_tensors else None
        below = ctx.down if _agg.takes_product_below(ctx.down, ctx.csr, c, ctx.k, b * nv, ctx.needs_input_grad[0]) else None
        grad_support, grad_bias = _agg.backward(None, ctx.csr, ctx.k, ctx.act, None, mask, *_bias_for(ctx),
                                                head=(gp, ctx.scale, ctx.shape), below=below)
        return (grad_support if ctx.needs_input_grad[0] else None), grad_bias, \
            (gp if ctx.needs_input_grad[2] else None), None, None, None, None, None


def zero_n_aggregate_head(support, adj, bias, k, activation, base, scale, down=None):
    """base + scale * zero_n_aggregate(...)[..., :3] for a [B,V,C] support: fused (see _ZeroNAggregateHead) for split-3
    layers on a bounded-degree mesh with ReLU or no activation, the two separate operators otherwise."""
    act, foreign, batched, csr = _route(activation, support, adj)
    if batched and not foreign and act != _ACT_ELU and csr.ell_w and k > 0 and k % 4 == 0 and support.shape[-1] == 3 * k:
        return _ZeroNAggregateHead.apply(support, bias, base, csr, k, act, scale, down)
    from .ops import VertexHead
    return VertexHead.apply(base, zero_n_aggregate(support, adj, bias, k, activation), scale)


def zero_n_aggregate(support, adj, bias, k, activation=None):
    """Shared tail of every 0N-GCN layer; accepts [V,C] or [B,V,C] support.  Returns the
    ACTIVATED output when `activation` is given (fused for relu / elu)."""
    act, foreign, _, csr = _route(activation, support, adj, any_input=True)
    if csr is None:
        # one dense adjacency PER MESH ([B,V,V]): what the reference's torch.matmul(adj, support[..., :k]) also accepts
        # (layers.py:111, 146).  Not a shape the reference drivers produce; served by the same dense product.
        out = torch.cat((torch.matmul(adj, support[..., :k]), support[..., k:]), dim=-1)
        if bias is not None:
            out = out + bias
        return out if activation is None else activation(out)
    s3 = support.unsqueeze(0) if support.dim() == 2 else support
    out = _ZeroNAggregate.apply(s3, bias, csr, k, act)
    if support.dim() == 2:
        out = out.squeeze(0)
    return activation(out) if foreign else out


# ---- a stack of layers with its layer BOUNDARIES as single launches (csrc/zn_stack.hip) -----------------------------------
# Between two consecutive 192-wide layers the aggregation of the first is the operand load of the second's product, and in the
# backward pass the aggregation backward of a layer is the operand load of its own input-gradient product.  The boundary
# launch does both; which boundaries take it is `fused.plan`'s decision (measured: it pays from ~6 meshes of 2562 vertices
# forward, ~10 backward).  The values are those of the separate operators: the aggregation's bit for bit, the products within
# fp32 summation order.
class _StackLink:
    """What two neighbouring launches of a stack hand each other outside autograd's edges: the boundary's forward launch
    leaves its weight transposed (`wt`); the launch ABOVE it in the backward pass (the next boundary's or the head's fused
    backward) computes this boundary's input gradient with it and leaves it in `dx`, stamped with the address of the support
    gradient it was computed from -- the boundary uses it only when that very tensor arrives as its incoming gradient (an
    engine that summed several consumers' gradients hands over another tensor, and the product is computed here as usual)."""
    __slots__ = ("wt", "dx", "g_ref", "wanted")

    def __init__(self):
        self.wt = self.dx = self.g_ref = None
        self.wanted = False

    def stamp(self, g):
        """`dx` was computed from the support gradient `g` as it is now (_identity.MemoryStamp: an engine that accumulates
        another consumer's gradient IN PLACE keeps the address and bumps the version)."""
        self.g_ref = MemoryStamp(g)

    def claim_dx(self, g):
        """The precomputed input gradient if `g` is the very memory (at the same version) it was computed from; one shot."""
        dx, stamp = self.dx, self.g_ref
        self.dx = self.g_ref = None
        return dx if dx is not None and stamp is not None and stamp.matches(g) else None

    def take_dx(self, b, nv):
        self.dx = torch.empty(b, nv, self.wt.shape[1], dtype=torch.float32, device=self.wt.device)
        return self.dx


class _FusedBoundary(torch.autograd.Function):
    """support_next = act([A . S[..., :k] | S[..., k:]] + bias) @ W_next -- layer L's aggregation and layer L+1's product."""

    @staticmethod
    def forward(ctx, support, bias, w_next, csr, k, act, up, down):
        s = _lib.require(support, "support", torch.float32, 3)
        c = s.shape[-1]
        bias_c = None if bias is None else _lib.require(bias, "bias", torch.float32, 1)
        w2 = w_next.reshape(w_next.shape[-2:])
        need = any(ctx.needs_input_grad[:3])
        mask = _agg.relu_mask(s, k) if need and act == _ACT_RELU else None
        if need:
            up.wt = torch.empty(w2.shape[1], c, dtype=torch.float32, device=s.device)
            up.wanted = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        x, s_next = _fused.layer_forward(s, bias_c, csr, k, act, w2, mask=mask, wt_out=up.wt)
        ctx.csr, ctx.k, ctx.act, ctx.up, ctx.down = csr, k, act, up, down
        ctx.bias_ref = _pass.parameter_ref(bias, ctx, ctx.needs_input_grad[1])
        ctx.w_ref = _pass.parameter_ref(w_next, ctx, ctx.needs_input_grad[2])
        ctx.masked = mask is not None
        ctx.save_for_backward(x, w_next, *([mask] if mask is not None else []))
        return s_next

    @staticmethod
    def backward(ctx, grad_next):
        x, w = ctx.saved_tensors[:2]
        mask = ctx.saved_tensors[2] if ctx.masked else None
        b, nv, c = x.shape
        rows = b * nv
        w2 = w.reshape(w.shape[-2:])
        n_out = w2.shape[1]
        g2 = grad_next.reshape(rows, n_out).contiguous()
        need_s, _, need_w = ctx.needs_input_grad[:3]
        need_b, bias = _bias_for(ctx)
        # ---- layer L+1's product: its gradients as after _dense (x is contiguous: saved by this node's forward), with dX taken from
        # the link when the launch above left it there, never postponed, and never on the any-shape kernel (the library, since
        # this product's forward was not that kernel's either)
        route = _products.route(rows, c, n_out, need_w, w2.is_contiguous(), True, False, _products._own_products_preferred(),
                                _products.use_any_shape_products)
        if route.dx == "any":
            route = route._replace(dx="lib")
        dx, grad_w = _products.product_gradients(x, g2, w, ctx.w_ref, route, need_s or need_b, need_w, dx=ctx.up.claim_dx(g2))
        if not (need_s or need_b):
            return None, None, grad_w, None, None, None, None, None
        # ---- layer L's aggregation: with the input gradient of ITS product in the same launch when the boundary below wants it
        below = ctx.down if _agg.takes_product_below(ctx.down, ctx.csr, c, ctx.k, rows, need_s) else None
        out = x if (ctx.act != _ACT_NONE and mask is None) else None
        grad_support, grad_bias = _agg.backward(dx, ctx.csr, ctx.k, ctx.act, out, mask, need_b, bias, below=below)
        return (grad_support if need_s else None), grad_bias, grad_w, None, None, None, None, None


# ---- the last layer of a stack that ends in positions, narrowed to the three columns that reach them ---------------------------
# zero_n_stack_positions returns base + scale * h[..., :3]: of the last layer's 192 output columns three are read, and its output
# gradient is [scale * grad_pos | 0 ...].  The wide route (product, _ZeroNAggregateHead, the pair launch of _Product) still
# writes a [rows, 192] output nobody reads and a [rows, 192] support gradient whose columns 3.. are zero, and multiplies those
# zeros through both gradient products.  _NarrowHead joins the product and the head in one node and keeps the live columns only;
# every tensor it hands on carries the wide route's bits (csrc/zn_gcn.hip "NARROW HEAD", csrc/dense_gemm.hip "NARROW pair").
# Used from NARROW_HEAD_MIN_ROWS rows: it moves fewer bytes at every size and the whole step is 7.6-9.4 % faster with it at 1, 2, 4
# and 8 meshes of 2562 vertices (profiles/r08_narrow_head.txt, section 3); the threshold keeps the small shapes on the launches
# their tests pin and goes no lower than the smallest multi-mesh shard measured (2 x 2562 rows).
NARROW_HEAD_MIN_ROWS = 4096

# None: the rule above, or the environment's GEOM_NARROW_HEAD = on | off;  "on" / "off": force the narrow route wherever the
# operands qualify, whatever the row count / the wide route everywhere (tests, A/B measurements of one tree)
narrow_head = None


def _narrow_head_mode():
    mode = narrow_head if narrow_head is not None else (os.environ.get("GEOM_NARROW_HEAD") or None)
    if mode not in (None, "on", "off"):
        raise ValueError("GEOM_NARROW_HEAD / layers.narrow_head must be 'on' or 'off' (got %r)" % (mode,))
    return mode


def _narrow_head_takes(h, layer, adj, activation, base):
    """Whether the last layer of a stack, applied to `h` with no fused boundary below it, takes _NarrowHead: exactly where the wide
    route is the fused head (zero_n_aggregate_head's rule) on a product routed Route(dx="pair", dw="split") of 192 x 192."""
    mode = _narrow_head_mode()
    if mode == "off" or current_slabs() is not None:
        return False
    w, bias = layer._weight(), layer.bias
    if not (torch.is_tensor(h) and h.dim() == 3 and layer.split == 3 and w.dim() in (2, 3) and tuple(w.shape[-2:]) == (192, 192)
            and (w.dim() == 2 or w.shape[0] == 1) and h.shape[-1] == 192):
        return False
    for t in (h, w, base) + (() if bias is None else (bias,)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == h.device):
            return False
    if not w.requires_grad or base.shape != h.shape[:-1] + (3,) or (bias is not None and bias.shape != (192,)):
        return False
    act, foreign, batched, csr = _route(activation, h, adj)
    if not batched or foreign or act == _ACT_ELU or not csr.ell_w or csr.nv != h.shape[1]:
        return False
    rows = h.shape[0] * h.shape[1]
    r = _products.route(rows, 192, 192, True, True, True, False, _products._own_products_preferred(), _products.use_any_shape_products)
    # (Route(dx="pair"): the input gradient is never the one a leaf has postponed to the end of the pass)
    return r.dx == "pair" and r.dw == "split" and (mode == "on" or rows >= NARROW_HEAD_MIN_ROWS)


class _NarrowHead(torch.autograd.Function):
    """positions = base + scale * act([A . S[..., :k] | S[..., k:]] + bias)[..., :3] with S = x @ W, k = 64: the last layer's
    product (the kernel `_dense` picks: S keeps its bits, and so do the positions) and its head in one node.  Backward: the
    head's backward on column group 0, then both gradients of the product from the [rows, 4] support gradient in one launch;
    weight and bias gradients go to the end-of-pass reduction as the wide nodes' do."""

    @staticmethod
    def forward(ctx, x, w, bias, base, csr, act, scale, forward_kind):
        w2 = w.reshape(w.shape[-2:])
        x, s = _products._forward(forward_kind, x, w2)
        if s.shape[1] != csr.nv:
            raise RuntimeError("support has %d vertices but the adjacency has %d" % (s.shape[1], csr.nv))
        pos = torch.empty_like(base)
        k = s.shape[-1] // 3
        sign = _agg.narrow_head_forward(s, bias, csr, k, act, base, scale, pos, want_sign=any(ctx.needs_input_grad[:3]))
        ctx.csr, ctx.k, ctx.act, ctx.scale = csr, k, act, float(scale)
        ctx.w_ref = _pass.parameter_ref(w, ctx, ctx.needs_input_grad[1])
        ctx.bias_ref = _pass.parameter_ref(bias, ctx, ctx.needs_input_grad[2])
        ctx.save_for_backward(x, w, *([sign] if sign is not None else []))
        return pos

    @staticmethod
    def backward(ctx, grad_pos):
        gp = grad_pos.contiguous()
        x, w = ctx.saved_tensors[:2]
        sign = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        need_x, need_w, need_b, need_base = ctx.needs_input_grad[:4]
        b, nv, cin = x.shape
        rows, c = b * nv, w.shape[-1]
        dx = grad_w = grad_bias = None
        if need_x or need_w or need_b:
            need_b = need_b and ctx.bias_ref is not None
            gs4, grad_bias = _agg.narrow_head_backward(gp, ctx.scale, sign, ctx.csr, ctx.k, ctx.act, (b, nv, c), need_b,
                                                       ctx.bias_ref() if need_b else None)
        if need_x or need_w:
            ws = _products._dense_kernels.weight_workspace(rows, cin, c, x.device)
            dx = torch.empty_like(x) if need_x else None
            _products._dense_kernels.backward_narrow(x.view(rows, cin), gs4, w.reshape(w.shape[-2:]), None if dx is None else dx.view(rows, cin), ws)
            if need_w:
                grad_w = _pass.weight_gradient(ctx.w_ref, w, rows, cin, c, ws)
        return dx, grad_w, grad_bias, (gp if need_base else None), None, None, None, None


def _narrow_head_positions(h, layer, adj, activation, base, scale):
    act, _, _, csr = _route(activation, h, adj)
    w = layer._weight()
    rows = h.shape[0] * h.shape[1]
    r = _products.route(rows, 192, 192, True, True, True, False, _products._own_products_preferred(), _products.use_any_shape_products)
    return _NarrowHead.apply(h, w, layer.bias, base, csr, act, scale, r.forward)


def _boundary_fuses(rows, csr, prev, layer):
    """Whether the boundary between `prev` and `layer` takes the single launch (csr: None unless the stack's input is batched
    and its activation one the kernels know)."""
    if not (current_slabs() is None and isinstance(csr, _Csr)):
        return False
    w = layer._weight()
    c = prev._weight().shape[-1]
    if w.dtype != torch.float32 or w.shape[-2] != c or not w.is_contiguous() or prev.split != 3 or c % 3:
        return False
    return _fused.supported(csr, c, c // 3, w.shape[-1]) and _fused.plan(rows)["fwd"]


def _stack_walk(x, adj, stack, activation, base=None):
    """The front of a stack: (support of its last layer, link of the last boundary, False) -- or, given the `base` of a
    coordinate update and a last layer that takes _NarrowHead, (INPUT of the last layer, None, True)."""
    act, foreign, _, csr = _route(activation, x, adj)
    if foreign:          # (a foreign callable is applied between the operators)
        csr = None
    if len(stack) == 1 and base is not None and _narrow_head_takes(x, stack[0], adj, activation, base):
        return x, None, True
    s = _dense(x, stack[0]._weight())
    link = None
    for prev, layer in zip(stack[:-1], stack[1:]):
        if _boundary_fuses(x.numel() // x.shape[-1], csr, prev, layer):
            up = _StackLink()
            s = _FusedBoundary.apply(s, prev.bias, layer._weight(), csr, _split_k(s, prev), act, up, link)
            link = up
        else:
            h = zero_n_aggregate(s, adj, prev.bias, _split_k(s, prev), activation)
            if layer is stack[-1] and base is not None and _narrow_head_takes(h, layer, adj, activation, base):
                return h, None, True
            s = _dense(h, layer._weight())
            link = None
    return s, link, False


def _stack_supports(x, adj, stack, activation):
    """The front of a stack up to the support of its last layer: (support, link of the last boundary)."""
    return _stack_walk(x, adj, stack, activation)[:2]


def zero_n_stack(x, adj, stack, activation):
    """stack[-1](... stack[1](stack[0](x, adj, activation), adj, activation) ...): consecutive 0N-GCN layers applied to one
    adjacency (GEOMetrics.py:117-131 runs such runs per deformation stage), their boundaries as single launches where
    `fused.plan` says so.  Same values as calling the layers one by one."""
    s, _ = _stack_supports(x, adj, stack, activation)
    return zero_n_aggregate(s, adj, stack[-1].bias, _split_k(s, stack[-1]), activation)


def zero_n_stack_positions(x, adj, stack, activation, base, scale):
    """base + scale * zero_n_stack(x, adj, stack, activation)[..., :3] -- the coordinate update of a deformation stage.  Where the
    last layer has no fused boundary below it and qualifies (_narrow_head_takes), only the three columns are computed of it."""
    s, link, narrow = _stack_walk(x, adj, stack, activation, base)
    if narrow:
        return _narrow_head_positions(s, stack[-1], adj, activation, base, scale)
    return zero_n_aggregate_head(s, adj, stack[-1].bias, _split_k(s, stack[-1]), activation, base, scale, down=link)


def _uniform(t, bound):
    t.data.uniform_(-bound, bound)


# ------------------------------------------------------------------ layers ----
class _ZeroNBase(Module):
    """Common body: `split` = denominator of the aggregated column fraction (10 or 3)."""
    split = 10

    def _weight(self):
        raise NotImplementedError

    def forward(self, input, adj, activation):
        support = _dense(input, self._weight())
        return zero_n_aggregate(support, adj, self.bias, _split_k(support, self), activation)

    def forward_positions(self, input, adj, activation, base, scale):
        """base + scale * self(input, adj, activation)[..., :3] -- the coordinate update of a deformation stage
        (GEOMetrics.py:121,126,131) without materialising the layer output's gradient (see zero_n_aggregate_head)."""
        if _narrow_head_takes(input, self, adj, activation, base):
            return _narrow_head_positions(input, self, adj, activation, base, scale)
        support = _dense(input, self._weight())
        return zero_n_aggregate_head(support, adj, self.bias, _split_k(support, self), activation, base, scale)


class ZERON_GCN(_ZeroNBase):
    """Unbatched layer, first C//10 output channels neighbour-aggregated (reference layers.py:14-41)."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = Parameter(torch.empty(in_features, out_features))
        if bias:
            self.bias = Parameter(torch.empty(out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _uniform(self.weight, 6.0 / math.sqrt(self.weight.size(0) + self.weight.size(1)))
        if self.bias is not None:
            self.bias.data.zero_()

    def _weight(self):
        return self.weight


class BatchZERON_GCN(ZERON_GCN):
    """Batched [B,V,Cin] input, same parameters and split (reference layers.py:121-152)."""


class Batch_Image_ZERON_GCNGCN(_ZeroNBase):
    """Batched layer with a [1,Cin,Cout] `weight1` and the first C//3 channels aggregated
    (reference layers.py:84-116; the initialiser's quirk of using size(0)==1 is kept)."""
    split = 3

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight1 = Parameter(torch.empty(1, in_features, out_features))
        if bias:
            self.bias = Parameter(torch.empty(out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _uniform(self.weight1, 0.3 * 6.0 / math.sqrt(self.weight1.size(1) + self.weight1.size(0)))
        if self.bias is not None:
            _uniform(self.bias, 0.1)

    def _weight(self):
        return self.weight1


class Image_ZERON_GCNGCN(_ZeroNBase):
    """Unbatched [V,Cin] input with a 2-D [Cin,Cout] `weight1` and the first C//3 channels aggregated (reference
    old_GEOMetrics/layers.py:106-149: the layer of the old driver's MeshDeformationBlock; state_dict keys and shapes are its
    checkpoints').  `adj`: the old driver's info dict (its 'adj' entry is taken), a dense [V,V] tensor or a _Csr.  The HIP
    operators are fp32 on the device; any other input (a CPU tensor, float64: what the fixtures are checked with) is evaluated
    with the reference's own expression on the dense adjacency."""
    split = 3

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight1 = Parameter(torch.empty(in_features, out_features))
        if bias:
            self.bias = Parameter(torch.empty(out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _uniform(self.weight1, 0.6 * 6.0 / math.sqrt(self.weight1.size(1) + self.weight1.size(0)))
        if self.bias is not None:
            _uniform(self.bias, 0.1)

    def _weight(self):
        return self.weight1

    def forward(self, input, adj, activation):
        adj = plain_adjacency(adj)
        if on_device_operators(input, adj):
            return super().forward(input, adj, activation)
        support = torch.mm(input, self.weight1)
        k = _split_k(support, self)
        output = torch.cat((torch.mm(adj, support[:, :k]), support[:, k:]), dim=1)
        if self.bias is not None:
            output = output + self.bias
        return activation(output)


def plain_adjacency(adj):
    """The adjacency an unbatched layer was given: the old driver hands its layers an info dict whose 'adj' entry it is."""
    return adj["adj"] if isinstance(adj, dict) else adj


def on_device_operators(input, adj):
    """Whether the HIP operators take an unbatched layer's call: an fp32 input on a HIP device with a _Csr or a dense fp32
    adjacency beside it."""
    if not (torch.is_tensor(input) and input.is_cuda and input.dtype == torch.float32):
        return False
    return isinstance(adj, _Csr) or (torch.is_tensor(adj) and adj.is_cuda)


class _MaxPoolBase(Module):
    """Aggregate like a 0N-GCN layer (split 10), then max over the vertex axis."""
    split = 10

    def __init__(self, in_features, print_length):
        super().__init__()
        self.in_features, self.print_length = in_features, print_length
        self.weight_Ws = nn.ParameterList([Parameter(torch.empty(in_features, print_length))])
        self.weight_Bs = nn.ParameterList([Parameter(torch.empty(print_length))])
        self.reset_parameters()

    def reset_parameters(self):
        _uniform(self.weight_Bs[0], 6.0 / math.sqrt(self.weight_Bs[0].size(0)))
        _uniform(self.weight_Ws[0], 6.0 / math.sqrt(self.weight_Ws[0].size(0) + self.weight_Ws[0].size(1)))

    def _pre_activation(self, r_s, adj):
        support = _dense(r_s, self.weight_Ws[0])
        return zero_n_aggregate(support, adj, self.weight_Bs[0], _split_k(support, self))


class GCNMax(_MaxPoolBase):
    """Unbatched: max over vertices of activation(v) (reference layers.py:43-79).  Given a RaggedMeshBatch as
    `adj` (r_s = the concatenated [sum(V), Cin] features) it returns one row per mesh, [B, print_length]."""

    def forward(self, r_s, adj, activation):
        support = _dense(r_s, self.weight_Ws[0])
        acted = zero_n_aggregate(support, adj, self.weight_Bs[0], _split_k(support, self), activation)
        if hasattr(adj, "offsets"):
            from .ops import SegmentMax
            return SegmentMax.apply(acted, adj.offsets, adj.max_len)
        return torch.max(acted, dim=0)[0]


class BatchGCNMax(_MaxPoolBase):
    """Batched: max over vertices of the PRE-activation values -- the reference computes the
    activation and then discards it (layers.py:186-187); preserved."""

    def forward(self, r_s, adj, activation):
        return torch.max(self._pre_activation(r_s, adj), dim=1)[0]
