"""The hidden layers of the mesh deformation block as ONE launch per layer and direction (csrc/deform_block.hip).

reference: models.py:237-297 -- `x = F.relu(self.bnK(self.gcK(features, adj, F.relu)))` thirteen times (gcK: layers.py:107-116,
bnK = nn.BatchNorm1d(verts)), `features = features + x; features /= 2` after every second layer.  As separate operators a
hidden layer is product -> aggregation -> per-vertex BatchNorm (three launches each way, the activation written and re-read
between them); here layer i's launch computes

    Z_i = aggregate(S_i) + bias_i ;  X_{i+1} = ReLU(BN_i(Z_i)) (+ residual, / 2) ;  S_{i+1} = X_{i+1} . W_{i+1}

and its backward launch the aggregation backward + input-gradient product of layer i + 1 and the BatchNorm backward of layer i.
The chain is one autograd node: its input is the FIRST layer's raw support S_1 = cat(features, pooled) . W_1 (that product and
its gradients stay with layers._dense), its output the block's final features X_14; the coordinate head gc15 stays the
existing layer.  Weight gradients of the twelve equal layers: one strided-batched product over the stacked activations and
support gradients; bias gradients: per-vertex column sums out of the backward launches, added up by one reduction.

Where every workgroup of a launch is resident at once (482 vertices on an MI355X: yes) the thirteen launches of a direction
are ONE (`chain`): a vertex's workgroup runs layer after layer and waits for its neighbours' rows inside the launch.

`SCHEDULE` is the block's layer plan (which layer averages with which earlier output, where a product follows, which outputs are
kept): every route walks it.  `serves()` says when the launches apply (`_servable`: 192-wide block, k = 64, bounded-degree table
of width 8, fp32 on a HIP device, BatchNorm over the input's vertices; and b <= 16, training mode, local BatchNorm
statistics); everything else takes the separate operators (models.py).  The one-launch chain also needs a structurally symmetric adjacency (`csr.symmetric_structure`); a directed one
takes the launches per layer.

Training batches of 17 .. 64 meshes (`serves_wide`, `wide_layer_forward` / `wide_layer_backward`): the same launch per layer and
direction with the vertex's batch rows as ceil(b / 16) <= 4 row tiles behind ONE register-resident weight slice
(geom_deform_layer_wide_{fwd,bwd}_f32); the vertex's statistics are combined across the tiles inside the workgroup.  Launches
per layer only -- never the one-launch chain, no counters.  Opt-in: `wide = True` (GEOM_DEFORM_WIDE=1); the default keeps the
separate operators above 16 meshes until the route has been timed against them.

Eval mode under no_grad (`serves_inference`, `inference_chain`): BatchNorm on the running statistics is a per-vertex affine map,
so the layer launch (geom_deform_infer_fwd_f32) tiles 16 consecutive rows of the flattened [B * V] rows instead of a vertex's
batch rows -- any batch, no cross-workgroup waits, nothing written to the BatchNorm state.

The BatchNorm-free block of the old driver (models.MeshDeformationBlock: `serves_plain`, `_PlainChain`, at the end of this
file): the same row tiling with a training backward (geom_deform_plain_{fwd,bwd}_f32), rows of any length -- split meshes.
"""
import collections
import ctypes
import os
import threading

import torch

from . import _lib
from . import layers as _layers

# models.py:252-292: which earlier activation a layer's output is averaged with.  Key: layer; value: "lead" (the leading 192
# columns of the block input) or j = X_j, the INPUT of layer j (X_{j} = output of layer j - 1).
RESIDUALS = {2: "lead", 4: 3, 6: 5, 8: 7, 10: 9, 12: 11, 13: 13}
LAYERS = 13
assert LAYERS <= _lib.DEFORM_CHAIN_MAX      # the chain launches take the whole block

# The block's hidden layers, one record per layer, in order -- what every route walks (the chain's forward and backward,
# inference_chain, the separate operators of models.py).  index: 1-based; residual: None, "lead" (the leading 192 columns of the
# block input) or j = the OUTPUT of layer j; product: the next layer's product follows in the layer's launch; head: the coordinate
# head may ride in it instead (the last layer); tap: a later layer reads the output as its residual, so it has to be kept.
Layer = collections.namedtuple("Layer", "index residual product head tap")
_SOURCE = {i: src if src == "lead" else src - 1 for i, src in RESIDUALS.items()}      # (X_j is the output of layer j - 1)
SCHEDULE = tuple(Layer(i, _SOURCE.get(i), i < LAYERS, i == LAYERS, i in _SOURCE.values()) for i in range(1, LAYERS + 1))

enabled = True      # tests / A-B timing: False keeps the separate operators
relu = True         # tests only: False drops the ReLU of every hidden layer (a smooth chain: every launch of the backward can then
#                     be held to a tight float64 bound -- under ReLU a pre-activation within rounding of zero may fall on either
#                     side in any two fp32 evaluations and switch a whole unit's term)


# rows * pitch (floats) of an operand the launches address with 32-bit byte offsets must stay below this
OFFSET_LIMIT = 2 ** 29


def hidden_layers(block):
    """(gc1..gc13, bn1..bn13) of a models.BatchMeshDeformationBlock."""
    return ([getattr(block, "gc%d" % i) for i in range(1, LAYERS + 1)], [getattr(block, "bn%d" % i) for i in range(1, LAYERS + 1)])


def _servable(block, features, pooled, csr):
    """What the training and the eval launches ask alike of a call of `block`, the cheap questions first: the package switch, a
    192-wide block, fp32 [B,V,*] inputs on a HIP device with b * nv * 192 < 2^29 (32-bit byte offsets), the bounded-degree table
    of width 8 (+ tail tables), and per layer a bias, the widths and fp32 BatchNorm tensors over the input's vertices (the
    launches index them by the input's vertex)."""
    if not enabled or block.hidden != 192:
        return False
    if not (features.is_cuda and features.dtype == torch.float32 and pooled.is_cuda and pooled.dtype == torch.float32
            and features.dim() == 3):
        return False
    if features.shape[0] * features.shape[1] * 192 >= OFFSET_LIMIT:
        return False
    if csr.ell_w != 8 or _tail_tables(csr) is False:
        return False
    for i, (gc, bn) in enumerate(zip(*hidden_layers(block))):
        if gc.bias is None or gc.weight1.shape[-1] != 192 or (i > 0 and gc.weight1.shape[-2] != 192):
            return False
        if bn.num_features != features.shape[1] or any(
                t is None or t.dtype != torch.float32 for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
            return False
    return True


def _serves_training(block, features, pooled, csr, lo, hi):
    """_servable in training mode with gradients, lo <= b <= hi meshes, local BatchNorm statistics with a momentum (each layer
    takes its own)."""
    if not block.training or not torch.is_grad_enabled() or (features.dim() == 3 and not lo <= features.shape[0] <= hi):
        return False
    return _servable(block, features, pooled, csr) and not any(
        bn._synchronised() or bn.momentum is None for bn in hidden_layers(block)[1])


def serves(block, features, pooled, csr):
    """Whether the fused training launches serve this call of `block` (a models.BatchMeshDeformationBlock): at most 16 meshes."""
    return _serves_training(block, features, pooled, csr, 0, 16)


# Training batches of 17 .. WIDE_MAX_BATCH meshes on the launches with ceil(b / 16) row tiles per vertex
# (geom_deform_layer_wide_*); False keeps the separate operators there.  OFF unless GEOM_DEFORM_WIDE=1: the route has not been
# timed against the separate operators yet (tools/time_deform_wide.py), and it goes on per batch only where that comparison
# shows a win beyond its spread.
wide = os.environ.get("GEOM_DEFORM_WIDE", "0") == "1"
WIDE_MAX_BATCH = _lib.DEFORM_WIDE_MAX_B


def serves_wide(block, features, pooled, csr):
    """Whether the wide training launches serve this call of `block`: the clauses of serves() with 17 <= b <= WIDE_MAX_BATCH
    meshes, and the `wide` switch."""
    return wide and features.dim() == 3 and _serves_training(block, features, pooled, csr, 17, WIDE_MAX_BATCH)


TAIL = _lib.DEFORM_TAIL      # entries of an adjacency row beyond the 8-wide neighbour table that the launches take


def _tail_tables(csr):
    """(tail_col, tail_val, tail_col_t, tail_val_t): the entries of every row beyond the neighbour table as a second,
    TAIL-wide table [nv, TAIL] (col -1 = padding) for A and A^T, or Nones where no row is longer; False when a row has more
    than 8 + TAIL entries (the launches then do not serve the adjacency).  Cached on the csr object."""
    cached = getattr(csr, "_deform_tail", None)
    if cached is not None:
        return cached
    out = []
    for over in (csr.over, csr.over_t):
        if over is None:
            out += [None, None]
            continue
        ptr, col, val = over
        lens = (ptr[1:] - ptr[:-1]).long()
        if int(lens.max()) > TAIL:
            csr._deform_tail = False
            return False
        nv = lens.numel()
        rows = torch.repeat_interleave(torch.arange(nv, device=col.device), lens)
        slot = torch.arange(col.numel(), device=col.device) - ptr[:-1].long()[rows]
        tcol = torch.full((nv, TAIL), -1, dtype=torch.int32, device=col.device)
        tval = torch.zeros((nv, TAIL), dtype=torch.float32, device=col.device)
        tcol[rows, slot] = col
        tval[rows, slot] = val
        out += [tcol.contiguous(), tval.contiguous()]
    csr._deform_tail = tuple(out)
    return csr._deform_tail


def pack_weights(weights, zero=None):
    """(fwd, bwd) [len(weights), 36864] each: every [192,192] weight (and its transpose) in the order a wave of the layer
    launches keeps its slice in registers -- ONE launch for all layers of a block (geom_deform_pack_weights_zero_f32).
    zero (optional int32 tensor): cleared by the same launch (the chain launches' counters)."""
    n = len(weights)
    w2 = [w.reshape(192, 192) if w.is_contiguous() else w.reshape(192, 192).contiguous() for w in weights]
    dev = w2[0].device
    fwd = torch.empty(n, 192 * 192, dtype=torch.float32, device=dev)
    bwd = torch.empty(n, 192 * 192, dtype=torch.float32, device=dev)
    _lib.call("geom_deform_pack_weights_zero_f32", n, w2, fwd, bwd, zero, 0 if zero is None else zero.numel())
    return fwd, bwd


# The hidden layers of a block as ONE launch per direction (geom_deform_chain_fwd_f32: a vertex's workgroup waits for its
# neighbours' rows inside the launch) where every workgroup of the launch is resident at once; False: one launch per layer.
#
# ONE chain launch at a time per device: a chain launch needs all its workgroups resident, and two of them that start together
# on two streams can each hold half of the chip and wait for the other half (the waits give up after seconds and the outputs
# are NaN -- loud, but a lost step).  A process therefore gives the chain launches of a device to ONE stream at a time: the
# stream that asks first owns them until it is idle, other streams issue the layers one by one meanwhile.  A stream that is being
# captured always records chain launches.  (Not covered: two PROCESSES sharing a GPU, and captured graphs replayed concurrently
# with other chain work -- set deform.chain = False (or GEOM_DEFORM_CHAIN=0 in the environment) there.)
chain = os.environ.get("GEOM_DEFORM_CHAIN", "1") != "0"
CTR_STRIDE = 32      # ints per vertex counter (one 128-byte line each)
_chain_owner = {}    # device index -> the torch stream that issues chain launches
_chain_lock = threading.Lock()


def chain_fits(nv, device):
    if not chain:
        return False
    with torch.cuda.device(device):      # (the occupancy query and the capture test are about the current device and stream)
        if not _lib.lib().geom_deform_chain_fits(int(nv)):
            return False
        mine = torch.cuda.current_stream(device)
        if torch.cuda.is_current_stream_capturing():
            return True      # (nothing runs now; whoever replays the graph keeps other chain work off the device meanwhile)
    with _chain_lock:
        owner = _chain_owner.get(device.index)
        if owner is None or owner == mine:
            _chain_owner[device.index] = mine
            return True
        try:                          # the owner has nothing in flight any more: the launches move to this stream
            idle = owner.query()
        except RuntimeError:          # (it is being captured)
            idle = False
        if idle:
            _chain_owner[device.index] = mine
        return idle


def _forward_args(s_in, bias, csr, bn_w, bn_b, run_mean, run_var, training, momentum, eps, relu, res, scale, z_out, x_out,
                  save_mean, save_invstd, w_next=None, s_out=None, w_head=None, s_head=None):
    b, nv, c = s_in.shape
    tail = _tail_tables(csr)
    return _lib.args(_lib.DeformFwd, b, nv, c, 64, csr.ell_w, s_in, bias, csr.ell_col, csr.ell_val, tail[0], tail[1], bn_w,
                     bn_b, run_mean, run_var, int(training), float(momentum), float(eps), int(relu), res,
                     res.stride(1) if res is not None else 0, float(scale), z_out, x_out, save_mean, save_invstd, w_next, s_out,
                     w_head, s_head, 0)


def layer_forward(s_in, *args, **kwargs):
    """One forward launch (geom_deform_layer_fwd_f32); w_next = the next layer's weight PACKED (pack_weights()[0][l]); see
    include/geom_hip.h for the operands."""
    _lib.call("geom_deform_layer_fwd_f32", _forward_args(s_in, *args, **kwargs))


def wide_layer_forward(s_in, *args, **kwargs):
    """layer_forward for 17 .. WIDE_MAX_BATCH meshes (geom_deform_layer_wide_fwd_f32): same arguments, same results."""
    _lib.call("geom_deform_layer_wide_fwd_f32", _forward_args(s_in, *args, **kwargs))


def chain_forward(layers, done):
    """`layers` (lists of layer_forward's arguments) as ONE launch (geom_deform_chain_fwd_f32); done: int32 [nv * CTR_STRIDE],
    zero."""
    _lib.call("geom_deform_chain_fwd_f32", len(layers), [_forward_args(*a, **k) for a, k in layers], done)


def rows_operand(t, shape, limit=None):
    """(tensor, row pitch in floats) of a [B,V,C] operand (a residual, a gradient) as the kernels read it: in place when it is
    fp32 on the device, row-major with contiguous rows at any pitch (a column slice of a wider buffer), a contiguous copy
    otherwise.  limit: the launch's bound on b * nv * pitch (OFFSET_LIMIT for a residual: its 32-bit byte offsets) -- a wider
    pitch that would reach it (the leading columns of a 963 / 1155-wide block input) is copied to pitch C, which the bound on
    b * nv * 192 that _servable checks keeps below it.  None -> (None, 0)."""
    if t is None:
        return None, 0
    b, nv, c = shape
    ok = (t.dim() == 3 and tuple(t.shape) == (b, nv, c) and t.is_cuda and t.dtype == torch.float32 and t.stride(2) == 1
          and t.stride(1) >= c and t.stride(0) == nv * t.stride(1) and t.data_ptr() % 4 == 0)
    if ok and limit is not None and b * nv * t.stride(1) >= limit:
        ok = False
    if not ok:
        t = t.contiguous()
    return t, t.stride(1)


def head_weight(head):
    """The coordinate head's weight ([1,192,3] / [192,3]: models.py:219 gc15) as the launches read it: [192, 3] contiguous."""
    return head.reshape(192, 3).contiguous()


def _backward_args(shape, csr, z, bn_w, bn_b, save_mean, save_invstd, relu, has_res, scale, dz, grad_bn_w, grad_bn_b,
                   dz_up=None, ds_up=None, wt_up=None, g=None, g2=None, grad_res=None, colsum=None, ds_head=None, w_head=None,
                   x_top=None, dw_head=None):
    """(struct, tensors it points into that were made here: the caller keeps them alive until the launch is issued)"""
    b, nv, c = shape
    tail = _tail_tables(csr)
    g, g_ld = rows_operand(g, shape)
    g2, g2_ld = rows_operand(g2, shape)
    a = _lib.args(_lib.DeformBwd, b, nv, c, 64, csr.ell_w, dz_up, csr.ell_col_t, csr.ell_val_t, tail[2], tail[3], ds_up, wt_up,
                  g, g2, g_ld, g2_ld, z, bn_w, bn_b, save_mean, save_invstd, int(relu), int(has_res), float(scale), grad_res,
                  dz, grad_bn_w, grad_bn_b, colsum, ds_head, w_head, x_top, dw_head, 0)
    return a, (g, g2)


def layer_backward(shape, csr, z, *args, **kwargs):
    """One backward launch (geom_deform_layer_bwd_f32); wt_up = the layer above's weight, TRANSPOSED and packed
    (pack_weights()[1][l])."""
    a, _keep = _backward_args(shape, csr, z, *args, **kwargs)
    _lib.call("geom_deform_layer_bwd_f32", a)


def wide_layer_backward(shape, csr, z, *args, **kwargs):
    """layer_backward for 17 .. WIDE_MAX_BATCH meshes (geom_deform_layer_wide_bwd_f32): same arguments, same results."""
    a, _keep = _backward_args(shape, csr, z, *args, **kwargs)
    _lib.call("geom_deform_layer_wide_bwd_f32", a)


def chain_backward(layers, done, ds_first=None):
    """`layers` (lists of layer_backward's arguments, the top layer first) as ONE launch (geom_deform_chain_bwd_f32); ds_first:
    receives the aggregation backward of the last layer's dZ (the chain's first layer has no activation behind its support)."""
    built = [_backward_args(*a, **k) for a, k in layers]
    _lib.call("geom_deform_chain_bwd_f32", len(built), [b[0] for b in built], done, ds_first)


def _stacked(xs):
    """x_out policy of _forward_walk: every layer's output is kept, layer i's in xs[i - 1] (a backward pass reads them)."""
    return lambda layer: xs[layer.index - 1]


def _dense_like(t):
    return torch.empty_like(t, memory_format=torch.contiguous_format)  # (the launches assume a pitch of 192)


def _rotating(like, out):
    """x_out policy of _forward_walk: only what a later launch or the caller reads is stored.  The outputs a residual taps
    (layer 2k's is the residual of layer 2k + 2, and layer 12's of layer 13) go to two buffers in turn, the last layer's to `out`."""
    bufs = (_dense_like(like), _dense_like(like))
    return lambda layer: out if layer.head else (bufs[(layer.index // 2) & 1] if layer.tap else None)


def _forward_walk(s1, lead, x_out_of, w2, w_head, s_head):
    """The forward walk over SCHEDULE that every route makes.  Yields per layer (layer, residual tensor or None, s_in, x_out,
    keywords): s_in = s1, then the two support buffers in turn; x_out = x_out_of(layer) (_stacked or _rotating), remembered for
    the layers whose residual it is; keywords = w_next (w2[i - 1], packed) / s_out where a product follows, w_head / s_head
    where the coordinate head rides in the launch."""
    s_buf = (_dense_like(s1), _dense_like(s1))
    kept = {}
    s_cur = s1
    for layer in SCHEDULE:
        i, src = layer.index, layer.residual
        res = None if src is None else (lead if src == "lead" else kept[src])
        x_out = x_out_of(layer)
        yield layer, res, s_cur, x_out, dict(w_next=w2[i - 1] if layer.product else None, s_out=s_buf[i & 1] if layer.product else None,
                                             w_head=w_head if layer.head else None, s_head=s_head if layer.head else None)
        if x_out is not None:
            kept[i] = x_out
        s_cur = s_buf[i & 1]


def _backward_walk(xs, wts, head, g_a, g_b, w_head, want_dw_head, partial_rows, emit, add=torch.add):
    """The backward walk over reversed(SCHEDULE) of both autograd nodes.  xs [13, *shape, 192] = the kept outputs, wts = the
    packed transposed weights; head: the node's second output is the coordinate head's raw support (g_b = its gradient) rather
    than a second handle on the features.  partial_rows: rows of a layer's bias-gradient (and head-weight) partials -- nv, or
    ceil(nv / 16) for the launches that write them per row-block.  emit(i, top, what) launches layer i (or collects it for a
    chain launch) with its own operands beside `what` (the keywords both launches share); add(a, b) joins two residual
    gradients that reach one layer.  Returns (dzs, dss, colsum, dw_head, g_lead)."""
    L = LAYERS
    shape, c = tuple(xs.shape[1:]), xs.shape[-1]
    f32 = dict(dtype=torch.float32, device=xs.device)
    ds_head = dw_head = None
    if head:                           # g_b is the gradient of the head's raw support
        if g_b is not None:
            ds_head = g_b.contiguous()
            dw_head = torch.empty(partial_rows, c * 3, **f32) if want_dw_head else None
        g_top, g_top2 = g_a, None
    else:
        g_top, g_top2 = (g_a, g_b) if g_a is not None else (g_b, None)      # (read in place at any row pitch)
    dzs = torch.empty(L, *shape, **f32)            # dzs[i - 1] = dZ_i
    dss = torch.empty(L - 1, *shape, **f32)        # dss[i - 2] = dS_i = gradient of layer i's raw support, i = 2..L
    colsum = torch.empty(L, partial_rows, c, **f32)
    pending = {}                                   # j -> gradient that reaches layer j's output through a residual average
    g_lead = None
    for i, src, _, top, _ in reversed(SCHEDULE):
        grad_res = torch.empty(*shape, **f32) if src is not None else None
        common = dict(dz=dzs[i - 1], grad_res=grad_res, colsum=colsum[i - 1])
        if top:
            what = dict(g=g_top, g2=g_top2, ds_head=ds_head, w_head=w_head if ds_head is not None else None,
                        x_top=xs[L - 1] if dw_head is not None else None, dw_head=dw_head, **common)
        else:
            what = dict(dz_up=dzs[i], ds_up=dss[i - 1], wt_up=wts[i - 1], g2=pending.pop(i, None), **common)
        emit(i, top, what)
        if src == "lead":
            g_lead = grad_res
        elif src is not None:
            pending[src] = add(pending[src], grad_res) if src in pending else grad_res
    assert not pending, "a residual gradient was left without its layer"
    return dzs, dss, colsum, dw_head, g_lead


def _reduce_gradients(xs, dss, colsum, dw_head):
    """The end of a backward pass: (bias gradients [13, 192], weight gradients [12, 192, 192], head-weight gradient [576] or
    None).  dW_i = X_i^T . dS_i, i = 2..L: one strided-batched product over the stacked activations and support gradients.
    Bias gradients: the launches' partial column sums added up in row order, all 13 layers and the head's [192, 3] partials in
    ONE launch (torch's reduction over the middle axis of [13, 482, 192] took 38 us; geom_colsum_batch_f32 is the reduction
    the aggregation backward's partials go through: fixed order, ~5 us)."""
    L = LAYERS
    c, parts = xs.shape[-1], colsum.shape[1]
    f32 = dict(dtype=torch.float32, device=xs.device)
    g_w = torch.bmm(xs[:L - 1].view(L - 1, -1, c).transpose(1, 2), dss.view(L - 1, -1, c))
    g_bias = torch.empty(L, c, **f32)
    jobs = [(colsum[i], c, g_bias[i]) for i in range(L)]
    g_head = None
    if dw_head is not None:
        g_head = torch.empty(c * 3, **f32)
        jobs.append((dw_head, c * 3, g_head))
    n = len(jobs)
    _lib.call("geom_colsum_batch_f32", n, [j[0] for j in jobs], (ctypes.c_int * n)(*([parts] * n)),
              (ctypes.c_int * n)(*[j[1] for j in jobs]), [j[2] for j in jobs])
    return g_bias, g_w, g_head


class _HiddenChain(torch.autograd.Function):
    """X_14 = the thirteen hidden layers applied to S_1 (see the module docstring).  apply(s1, lead, csr, stats, momentum,
    eps, *biases[13], *weights[12] (gc2..gc13), *bn_weights[13], *bn_biases[13]); stats = [(running_mean, running_var)] * 13,
    momentum / eps = the 13 BatchNorms' own values (sequences of 13).
    Returns the final features TWICE (two tensor objects over one memory: one for the coordinate head, one for the caller;
    their gradients meet inside the first backward launch instead of in an add pass)."""

    @staticmethod
    def forward(ctx, s1, lead, csr, stats, momentum, eps, w_head, *params):
        """w_head: the coordinate head's weight ([1,192,3] / [192,3]: models.py:219 gc15) or None.  Given, the head's product
        rides in the last layer's launch and the SECOND output is its raw support [B,V,3] (the caller aggregates it and adds
        the bias) instead of a second handle on the features."""
        L = LAYERS
        biases, weights = params[:L], params[L:2 * L - 1]
        bn_w, bn_b = params[2 * L - 1:3 * L - 1], params[3 * L - 1:4 * L - 1]
        s1 = _lib.require(s1, "s1", torch.float32, 3, 192)
        # in place when it is the leading columns of the block's wide input (a copy where its byte offsets would pass 32 bits)
        lead, _ = rows_operand(lead, tuple(s1.shape), OFFSET_LIMIT)
        b, nv, c = s1.shape
        dev = s1.device
        f32 = dict(dtype=torch.float32, device=dev)
        xs = torch.empty(L, b, nv, c, **f32)          # xs[i - 1] = X_{i+1}, the output of layer i
        zs = torch.empty(L, b, nv, c, **f32)          # zs[i - 1] = Z_i, what BN_i normalised
        means, invstds = torch.empty(L, nv, **f32), torch.empty(L, nv, **f32)
        # (a chain launch needs a symmetric pattern: vertex v rewrites its support row once the vertices of ITS row are done
        # with the previous layer, and those must be all the vertices that gather v's row -- A[u][v] != 0 => A[v][u] != 0)
        # (above 16 meshes: the wide launches, layer by layer -- never a chain, no counters)
        as_chain = b <= 16 and csr.symmetric_structure and chain_fits(nv, dev)
        forward_launch = layer_forward if b <= 16 else wide_layer_forward
        # (counters of the forward and of the backward chain launch, cleared by the packing launch)
        counters = torch.empty(2, nv * CTR_STRIDE, dtype=torch.int32, device=dev) if as_chain else None
        w2, wts = pack_weights(weights, counters)     # w2[i - 1] / wts[i - 1] = W_{i+1} / its transpose, in register-slice order
        calls = []
        wh = s_head = None
        if w_head is not None:
            wh, s_head = head_weight(w_head), torch.empty(b, nv, 3, **f32)
        for layer, res, s_in, x_out, kw in _forward_walk(s1, lead, _stacked(xs), w2, wh, s_head):
            i = layer.index
            call = ((s_in, biases[i - 1], csr, bn_w[i - 1], bn_b[i - 1], stats[i - 1][0], stats[i - 1][1], True, momentum[i - 1],
                     eps[i - 1], relu, res, 0.5, zs[i - 1], x_out, means[i - 1], invstds[i - 1]), kw)
            if as_chain:
                calls.append(call)
            else:
                forward_launch(*call[0], **call[1])
        if as_chain:
            chain_forward(calls, counters[0])
        ctx.counters = counters[1] if as_chain else None
        ctx.csr, ctx.relu, ctx.head = csr, relu, w_head is not None
        ctx.head_shape = None if w_head is None else tuple(w_head.shape)
        ctx.set_materialize_grads(False)      # a handle nobody uses (the last block's features) arrives as None, not as 5.9 MB of zeros
        ctx.save_for_backward(xs, zs, means, invstds, wts, *bn_w, *bn_b, *([wh] if w_head is not None else []))
        out = xs[L - 1]
        return (out, s_head) if w_head is not None else (out, _layers._alias(out))

    @staticmethod
    def backward(ctx, g_a, g_b):
        L = LAYERS
        saved = ctx.saved_tensors
        xs, zs, means, invstds, wts = saved[:5]
        bn_w, bn_b = saved[5:5 + L], saved[5 + L:5 + 2 * L]
        csr = ctx.csr
        _, b, nv, c = xs.shape
        dev = xs.device
        f32 = dict(dtype=torch.float32, device=dev)
        n_in = 7 + 4 * L - 1
        if g_a is None and g_b is None:
            return (None,) * n_in
        w_head = saved[5 + 2 * L] if ctx.head else None
        g_bnw, g_bnb = torch.empty(L, nv, **f32), torch.empty(L, nv, **f32)
        # (the forward ran as one launch: so does the backward, if this stream still owns the device's chain launches)
        counters = ctx.counters
        # (its counters are good for ONE pass: a second backward over a retained graph takes the launches per layer)
        calls = [] if ctx.counters is not None and chain_fits(nv, dev) else None
        if calls is not None:
            ctx.counters = None
        backward_launch = layer_backward if b <= 16 else wide_layer_backward

        def emit(i, top, what):
            where = ((b, nv, c), csr, zs[i - 1], bn_w[i - 1], bn_b[i - 1], means[i - 1], invstds[i - 1])
            what = dict(what, relu=ctx.relu, has_res=SCHEDULE[i - 1].residual is not None, scale=0.5, grad_bn_w=g_bnw[i - 1],
                        grad_bn_b=g_bnb[i - 1])
            if calls is None:
                backward_launch(*where, **what)
            else:
                calls.append((where, what))

        def add(first, second):
            if calls is not None:
                raise RuntimeError("two residual gradients for one layer: not expressible inside one launch")
            return first + second

        dzs, dss, colsum, dw_head, g_lead = _backward_walk(xs, wts, ctx.head, g_a, g_b, w_head, ctx.needs_input_grad[6], nv, emit, add)
        # dS_1 = aggregation backward of the first layer (no activation between S_1 and Z_1): a last step of the chain launch, or
        # the existing operator
        if calls is not None:
            g_s1 = torch.empty(b, nv, c, **f32)
            chain_backward(calls, counters, ds_first=g_s1)
        else:
            g_s1, _ = _layers.aggregate_backward(dzs[0], csr, 64, _layers._ACT_NONE, None, None, False)
        g_bias, g_w, g_head = _reduce_gradients(xs, dss, colsum, dw_head)
        grads = [g_bias[i] for i in range(L)] + [g_w[i].view(1, c, c) for i in range(L - 1)] \
            + [g_bnw[i] for i in range(L)] + [g_bnb[i] for i in range(L)]
        g_wh = None if g_head is None else g_head.view(ctx.head_shape)
        return (g_s1, g_lead, None, None, None, None, g_wh, *grads)


def serves_inference(block, features, pooled, csr):
    """Whether the eval-mode launches (geom_deform_infer_fwd_f32) serve this call of `block`: eval() under no_grad, a
    192-wide block, fp32 on a HIP device, the bounded-degree table, and biases / BatchNorm parameters and running statistics
    in fp32 over the input's vertices.  No limit on the batch but b * nv * 192 < 2^29 (the 32-bit byte offsets of the
    launches' [b, nv, 192] operands; infer_layer_forward copies a wider residual to that pitch where it would pass them), no
    symmetry requirement on the adjacency (no workgroup waits for another) and no BatchNorm synchronisation (eval mode has no
    batch statistics)."""
    if block.training or torch.is_grad_enabled() or (features.dim() == 3 and features.shape[0] < 1):
        return False
    return _servable(block, features, pooled, csr)


def infer_layer_forward(s_in, bias, csr, bn_w, bn_b, run_mean, run_var, eps, relu, res, scale, x_out, w_next=None, s_out=None,
                        w_head=None, s_head=None):
    """One eval-mode launch (geom_deform_infer_fwd_f32): x_out (may be None) = relu?(BN_eval(aggregate(s_in) + bias))
    (+ res, * scale); s_out = x_out . W_next (w_next PACKED: pack_weights()[0][l]) or, on the last layer, s_head = x_out . w_head."""
    b, nv, c = s_in.shape
    tail = _tail_tables(csr)
    res, res_ld = rows_operand(res, (b, nv, c), OFFSET_LIMIT)
    a = _lib.args(_lib.DeformInfer, b, nv, c, 64, csr.ell_w, s_in, bias, csr.ell_col, csr.ell_val, tail[0], tail[1], bn_w, bn_b,
                  run_mean, run_var, float(eps), int(relu), res, res_ld, float(scale), x_out, w_next, s_out, w_head, s_head)
    _lib.call("geom_deform_infer_fwd_f32", a)


def inference_chain(block, s1, lead, csr, head=None):
    """The thirteen hidden layers of `block` in eval mode applied to the first layer's raw support s1 [B,V,192]: one packing
    launch and thirteen geom_deform_infer_fwd_f32 launches.  Returns (features, features, head_support) as hidden_chain does:
    head_support = the raw support [B,V,3] of `head` (the block's 192 -> 3 coordinate layer) when it is given, else None.
    Writes nothing to the BatchNorms' running statistics; only the activations a residual or the caller reads are stored."""
    s1 = _lib.require(s1, "s1", torch.float32, 3, 192)
    b, nv, c = s1.shape
    dev = s1.device
    f32 = dict(dtype=torch.float32, device=dev)
    gcs, bns = hidden_layers(block)
    w2, _ = pack_weights([g.weight1 for g in gcs[1:]])
    out = torch.empty(b, nv, c, **f32)
    wh = s_head = None
    if head is not None:
        wh, s_head = head_weight(head.weight1), torch.empty(b, nv, 3, **f32)
    for layer, res, s_in, x_out, kw in _forward_walk(s1, lead, _rotating(s1, out), w2, wh, s_head):
        gc, bn = gcs[layer.index - 1], bns[layer.index - 1]
        infer_layer_forward(s_in, gc.bias, csr, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, relu, res, 0.5, x_out, **kw)
    return out, out, s_head


def hidden_chain(block, s1, lead, csr, head=None):
    """The thirteen hidden layers of `block` applied to the first layer's raw support; returns (features for the coordinate
    layer, features for the caller, None) -- two handles, see _HiddenChain -- or, with head = the block's coordinate layer
    (192 -> 3 with a bias: the caller's decision), (features, the same, raw support of the head)."""
    gcs, bns = hidden_layers(block)
    for bn in bns:
        bn._pending_batches += 1
    stats = [(bn.running_mean, bn.running_var) for bn in bns]
    params = [g.bias for g in gcs] + [g.weight1 for g in gcs[1:]] + [bn.weight for bn in bns] + [bn.bias for bn in bns]
    momentum, eps = tuple(float(bn.momentum) for bn in bns), tuple(float(bn.eps) for bn in bns)
    if head is None:
        return _HiddenChain.apply(s1, lead, csr, stats, momentum, eps, None, *params) + (None,)
    feats, s_head = _HiddenChain.apply(s1, lead, csr, stats, momentum, eps, head.weight1, *params)
    return feats, feats, s_head


# ---- the BatchNorm-free block of the old driver on split meshes (models.MeshDeformationBlock; reference models.py:138-201) ----
# One launch per hidden layer and direction (geom_deform_plain_{fwd,bwd}_f32): rows of any length, any vertex count, no
# condition on the adjacency's table width or symmetry.  ON: one block's eager forward + backward takes 1.59 ms against 3.23
# (482 vertices) and 1.20 ms against 2.61 (1442 vertices after a split of every face) for the separate operators, beyond the
# run-to-run spread at both (tools/time_plain_block.py, profiles/plain_block.txt); GEOM_DEFORM_PLAIN=0 keeps the separate operators.
plain = os.environ.get("GEOM_DEFORM_PLAIN", "1") != "0"


def plain_layers(block):
    """gc1..gc13 of a models.MeshDeformationBlock."""
    return [getattr(block, "gc%d" % i) for i in range(1, LAYERS + 1)]


def plain_head(block):
    """The block's coordinate layer where its product rides in the launches (192 -> 3 with a bias), else None."""
    head = block.gc15
    return head if tuple(head.weight1.shape) == (192, 3) and head.bias is not None else None


def serves_plain(block, features, pooled, csr):
    """Whether the launches serve this call of `block` (a models.MeshDeformationBlock), the cheap questions first: the
    switches, a 192-wide block, fp32 [V,*] inputs on a HIP device with nv * 192 < 2^29 (32-bit byte offsets), and per hidden
    layer a bias and the 192 widths.  Nothing is asked of the adjacency: any table width, any row length, any pattern."""
    if not (enabled and plain) or block.hidden != 192:
        return False
    if not (torch.is_tensor(features) and torch.is_tensor(pooled) and features.is_cuda and pooled.is_cuda
            and features.dtype == torch.float32 and pooled.dtype == torch.float32 and features.dim() == 2 and pooled.dim() == 2):
        return False
    if features.shape[0] < 1 or features.shape[0] * 192 >= OFFSET_LIMIT:
        return False
    for i, gc in enumerate(plain_layers(block)):
        w = gc.weight1
        if gc.bias is None or w.dtype != torch.float32 or w.shape[-1] != 192 or (i > 0 and w.shape[-2] != 192):
            return False
    return True


def plain_tables(csr):
    """((ell_col, ell_val, over), (ell_col_t, ell_val_t, over_t)) of A and A^T at table width 8 -- layers._to_ell, whatever
    csr.ell_w is; over = (ptr, col, val) of the rows' entries beyond the table, or None.  Cached on the csr object."""
    cached = getattr(csr, "_deform_plain", None)
    if cached is None:
        with torch.no_grad():
            cached = (_layers._to_ell(csr.rowptr, csr.col, csr.val, 8), _layers._to_ell(csr.rowptr_t, csr.col_t, csr.val_t, 8))
        csr._deform_plain = cached
    return cached


def plain_layer_forward(s_in, bias, csr, relu, res, scale, z_out=None, x_out=None, w_next=None, s_out=None, w_head=None, s_head=None):
    """One forward launch (geom_deform_plain_fwd_f32) over s_in [b,nv,192] or [nv,192]; w_next PACKED (pack_weights()[0][l]);
    see include/geom_hip.h for the operands."""
    b, nv = (1, s_in.shape[0]) if s_in.dim() == 2 else s_in.shape[:2]
    (col, val, over), _ = plain_tables(csr)
    over = over or (None, None, None)
    res, res_ld = rows_operand(None if res is None else res.reshape(b, nv, -1), (b, nv, 192), OFFSET_LIMIT)
    a = _lib.args(_lib.DeformPlainFwd, b, nv, 192, 64, s_in, bias, col, val, over[0], over[1], over[2], int(relu), res, res_ld,
                  float(scale), z_out, x_out, w_next, s_out, w_head, s_head)
    _lib.call("geom_deform_plain_fwd_f32", a)


def plain_layer_backward(shape, csr, z, relu, has_res, scale, dz, dz_up=None, ds_up=None, wt_up=None, g=None, g2=None, grad_res=None,
                         colsum=None, ds_head=None, w_head=None, x_top=None, dw_head=None):
    """One backward launch (geom_deform_plain_bwd_f32) over `shape` = (b, nv, 192); wt_up = the layer above's weight,
    TRANSPOSED and packed (pack_weights()[1][l]); colsum [ceil(b nv / 16), 192] and dw_head [ceil(b nv / 16), 576]."""
    b, nv, c = shape
    _, (col_t, val_t, over_t) = plain_tables(csr)
    over_t = over_t or (None, None, None)
    g, g_ld = rows_operand(None if g is None else g.reshape(b, nv, -1), shape, OFFSET_LIMIT)
    g2, g2_ld = rows_operand(None if g2 is None else g2.reshape(b, nv, -1), shape, OFFSET_LIMIT)
    product = dz_up is not None
    a = _lib.args(_lib.DeformPlainBwd, b, nv, c, 64, dz_up, col_t if product else None, val_t if product else None,
                  over_t[0] if product else None, over_t[1] if product else None, over_t[2] if product else None, ds_up, wt_up,
                  g, g2, g_ld, g2_ld, z, int(relu), int(has_res), float(scale), grad_res, dz, colsum, ds_head, w_head, x_top, dw_head)
    _lib.call("geom_deform_plain_bwd_f32", a)


class _PlainChain(torch.autograd.Function):
    """X_14 = the thirteen hidden layers of a models.MeshDeformationBlock applied to S_1 [V,192], and the raw support of its
    coordinate head: apply(s1, lead, csr, w_head, *biases[13], *weights[12] (gc2..gc13)) -> (features [V,192], s_head [V,3]
    or a second handle on the features when w_head is None).  _HiddenChain without the BatchNorm: one launch per layer and
    direction, Z and X' kept for the backward only when a gradient is wanted."""

    @staticmethod
    def forward(ctx, s1, lead, csr, w_head, *params):
        L = LAYERS
        biases, weights = params[:L], params[L:2 * L - 1]
        s1 = _lib.require(s1, "s1", torch.float32, 2, 192)
        nv, c = s1.shape
        if nv != csr.nv:
            raise RuntimeError("support has %d vertices but the adjacency has %d" % (nv, csr.nv))
        lead3, _ = rows_operand(lead.unsqueeze(0), (1, nv, c), OFFSET_LIMIT)
        f32 = dict(dtype=torch.float32, device=s1.device)
        train = any(ctx.needs_input_grad)
        # with gradients every layer's Z (the mask: X' loses it under a residual) and X' (the weight gradients) are kept;
        # without, only what a later launch reads (_rotating)
        xs = torch.empty(L, nv, c, **f32) if train else None
        zs = torch.empty(L, nv, c, **f32) if train else None
        out = xs[L - 1] if train else torch.empty(nv, c, **f32)
        w2, wts = pack_weights(weights)     # w2[i - 1] / wts[i - 1] = W_{i+1} / its transpose, in register-slice order
        wh = s_head = None
        if w_head is not None:
            wh, s_head = head_weight(w_head), torch.empty(nv, 3, **f32)
        for layer, res, s_in, x_out, kw in _forward_walk(s1, lead3, _stacked(xs) if train else _rotating(s1, out), w2, wh, s_head):
            i = layer.index
            plain_layer_forward(s_in, biases[i - 1], csr, relu, res, 0.5, z_out=zs[i - 1] if train else None, x_out=x_out, **kw)
        ctx.csr, ctx.relu, ctx.head = csr, relu, w_head is not None
        ctx.head_shape = None if w_head is None else tuple(w_head.shape)
        ctx.set_materialize_grads(False)
        if train:
            ctx.save_for_backward(xs, zs, wts, *([wh] if w_head is not None else []))
        return (out, s_head) if w_head is not None else (out, _layers._alias(out))

    @staticmethod
    def backward(ctx, g_a, g_b):
        L = LAYERS
        xs, zs, wts = ctx.saved_tensors[:3]
        csr = ctx.csr
        _, nv, c = xs.shape
        n_in = 4 + 2 * L - 1
        if g_a is None and g_b is None:
            return (None,) * n_in
        w_head = ctx.saved_tensors[3] if ctx.head else None

        def emit(i, top, what):
            plain_layer_backward((1, nv, c), csr, zs[i - 1], ctx.relu, SCHEDULE[i - 1].residual is not None, 0.5, **what)

        # (the launches write the bias-gradient and head-weight partials per row-block)
        dzs, dss, colsum, dw_head, g_lead = _backward_walk(xs, wts, ctx.head, g_a, g_b, w_head, ctx.needs_input_grad[3], (nv + 15) // 16, emit)
        # dS_1 = aggregation backward of the first layer (no activation between S_1 and Z_1): the existing operator
        g_s1, _ = _layers.aggregate_backward(dzs[0].unsqueeze(0), csr, 64, _layers._ACT_NONE, None, None, False)
        g_bias, g_w, g_head = _reduce_gradients(xs, dss, colsum, dw_head)
        grads = [g_bias[i] for i in range(L)] + [g_w[i] for i in range(L - 1)]
        g_wh = None if g_head is None else g_head.view(ctx.head_shape)
        return (g_s1.view(nv, c), g_lead, None, g_wh, *grads)


def plain_chain(block, s1, lead, csr, head=None):
    """The thirteen hidden layers of `block` applied to the first layer's raw support: (features, raw support of `head` or
    None)."""
    gcs = plain_layers(block)
    params = [g.bias for g in gcs] + [g.weight1 for g in gcs[1:]]
    feats, second = _PlainChain.apply(s1, lead, csr, None if head is None else head.weight1, *params)
    return feats, (second if head is not None else None)
