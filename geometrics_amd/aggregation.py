"""The launches of the 0N-GCN aggregation out = act([A . S[..., :k] | S[..., k:]] + bias) (csrc/zn_gcn.hip): one forward and one
backward launcher for the plain aggregation, the head, and the backward that takes the product below along (csrc/zn_stack.hip).
The table-or-CSR choice, the table's tail, the sign mask and the bias gradient's buffer, scratch and reduction are written here."""
import torch
import torch.nn.functional as F

from . import _lib
from . import backward_pass as _pass
from . import fused as _fused
from .products import _new_like

ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2


def activation_code(activation):
    """ReLU / ELU(alpha=1) are folded into the kernel epilogue (and their derivative into the
    backward read); any other callable is applied by the caller after an un-activated kernel."""
    if activation is F.relu or activation is torch.relu:
        return ACT_RELU
    if activation is F.elu:
        return ACT_ELU
    return ACT_NONE


def relu_mask(s, k):
    """One sign bit per output element: the backward takes relu' from it instead of re-reading `out`.  None: no mask path."""
    words = _lib.lib().geom_zn_gcn_relu_mask_words(*s.shape, k)
    return torch.empty(words, dtype=torch.int16, device=s.device) if words else None


def _table(csr, transposed):
    """The table arguments of an entry point: width, columns, values, and the CSR tail of the rows longer than the table."""
    col, val, over = (csr.ell_col_t, csr.ell_val_t, csr.over_t) if transposed else (csr.ell_col, csr.ell_val, csr.over)
    return (csr.ell_w, col, val) + tuple(over or (None, None, None))


def _table_took(csr, name, *args):
    """Launch a table entry point that has a CSR counterpart; False: there is no table, or the library's route refuses the shape."""
    code = _lib.status(name, *args) if csr.ell_w else _lib.EUNSUPPORTED
    if code != _lib.EUNSUPPORTED:
        _lib.check(code, name)
    return code != _lib.EUNSUPPORTED


def forward(s, bias_c, csr, k, act, out, want_mask=False, head=None):
    """Launch out = act([A . s[..., :k] | s[..., k:]] + bias) on contiguous fp32 [B,V,C] tensors: the fixed-stride table
    kernel when the adjacency has one (bounded degrees; long rows continue in its CSR tail), the generic CSR kernel
    otherwise.  head = (base, scale, pos): pos = base + scale * out[..., :3] out of the same launch (table kernel only: a
    refusal is an error).  Returns the ReLU sign mask when one was asked for and written."""
    b, nv, c = s.shape
    mask = relu_mask(s, k) if want_mask and act == ACT_RELU and csr.ell_w else None
    operands = (s, bias_c, act, out)
    if head is not None:
        base, scale, pos = head
        _lib.call("geom_zn_gcn_aggregate_ell_head_fwd_f32", b, nv, c, k, *_table(csr, False), *operands, mask, base, float(scale), pos)
    elif not _table_took(csr, "geom_zn_gcn_aggregate_ell_fwd_f32", b, nv, c, k, *_table(csr, False), *operands, mask):
        mask = None
        _lib.call("geom_zn_gcn_aggregate_fwd_f32", b, nv, c, k, csr.rowptr, csr.col, csr.val, *operands)
    return mask


def takes_product_below(below, csr, c, k, rows, needs_support):
    """Whether the aggregation backward of a [rows, c] layer also computes the input gradient of the product below it
    (`below`: the _StackLink of the boundary that produced this layer's support): wanted -- that boundary needs a gradient,
    this layer's support too, `fused.plan` says it pays -- and a shape the boundary kernel serves.

    _FusedBoundary.backward used to ask only for `below.wt`, `below.wanted` and the plan.  Between two boundaries that is the
    same answer: the node exists only where `_boundary_fuses` found supported(csr, c, k, .); `below.wt` was made by the
    boundary below as [its n_out, its c] -- 2-d, its n_out the width of the support it handed this node (= c), its c = 192
    since it was supported too -- and `below.wanted` means its output, this node's support, needs a gradient.  The head is
    where the long form decides: it runs at any split-3 width, e.g. 48 behind a fused 192 -> 48 boundary."""
    return bool(below is not None and below.wt is not None and below.wanted and needs_support and _fused.plan(rows)["bwd"]
                and below.wt.dim() == 2 and below.wt.shape[0] == c and _fused.supported(csr, c, k, below.wt.shape[1]))


def backward(g, csr, k, act, out, mask, want_bias, bias=None, arena=None, head=None, below=None):
    """grad_support = [A^T . g'[..., :k] | g'[..., k:]] with g' = g * act'(out) (relu' from the sign mask when there is
    one), and the bias gradient = column sums of g' out of the same launch (+ a fixed-order reduction: at once, or -- given
    the bias parameter, inside a backward pass -- batched at the end of the pass: geometrics_amd.backward_pass).
    head = (grad_pos, scale, (b, nv, c)): g is [scale * grad_pos | 0 ...] by construction, never materialised (pass None);
    below: a link for which takes_product_below() holds -- that product's input gradient is left in it."""
    grad_pos, scale, (b, nv, c) = head if head is not None else (None, 0.0, g.shape)
    device = g.device if head is None else grad_pos.device
    grad_support = _new_like(g, "grad_support", arena, descending=True) if head is None \
        else torch.empty(b, nv, c, dtype=torch.float32, device=device)
    # column sums of g' come out of the same kernel as per-workgroup partials (+ fixed-order reduce)
    rows = _fused.partial_rows(b, nv) if below is not None else None
    bg = _pass.NO_BIAS_GRADIENT
    if want_bias:
        scratch = (rows, c) if below is not None else _lib.lib().geom_zn_gcn_bwd_scratch_floats(b, nv, c)
        bg = _pass.bias_gradient(bias, c, device, scratch, opted_in=arena is not None)
    ell_w = csr.ell_w
    results = (grad_support, bg.now, bg.scratch)
    if below is not None:      # (the boundary below picks its input gradient up from the link instead of computing it)
        _fused.layer_backward(g, out, mask, csr, k, act, below.wt, g_out=grad_support, grad_in=below.take_dx(b, nv),
                              colsum_partial=bg.scratch, grad_pos=grad_pos, head_scale=scale, shape=(b, nv, c))
        below.stamp(grad_support)
    elif head is not None:
        _lib.call("geom_zn_gcn_aggregate_ell_head_bwd_f32", b, nv, c, k, *_table(csr, True), grad_pos, scale, mask, act, *results)
    elif not _table_took(csr, "geom_zn_gcn_aggregate_ell_bwd_f32", b, nv, c, k, *_table(csr, True), g, out, mask, act, *results):
        ell_w = 0
        _lib.call("geom_zn_gcn_aggregate_bwd_f32", b, nv, c, k, csr.rowptr_t, csr.col_t, csr.val_t, g, out, act, *results)
    if below is not None:          # the boundary kernel never reduces its partials itself
        bg.finish(rows)
    elif bg.defer:
        bg.finish(int(_lib.lib().geom_zn_gcn_bwd_partial_rows(b, nv, c, k, ell_w)))
    return grad_support, bg.out


# ---- the narrow head: the head layer of a stack, of whose output only the three position columns are ever read -------------
def narrow_head_forward(s, bias_c, csr, k, act, base, scale, pos, want_sign):
    """pos = base + scale * act([A . s[..., :k] | ...] + bias)[..., :3] from column group 0 of the rows alone -- the wide head's
    steps in its order, so its bits; no [B,V,C] output.  Returns the ReLU sign words ([B*V] int16) when asked for, else None."""
    b, nv, c = s.shape
    sign = torch.empty(b * nv, dtype=torch.int16, device=s.device) if want_sign and act == ACT_RELU else None
    _lib.call("geom_zn_gcn_narrow_head_fwd_f32", b, nv, c, k, *_table(csr, False), s, bias_c, act, base, float(scale), pos, sign)
    return sign


def narrow_head_backward(grad_pos, scale, sign, csr, k, act, shape, want_bias, bias=None):
    """(columns 0..3 of the wide head's support gradient as [B*V, 4] -- its other columns are zero -- and the bias gradient,
    whose partials keep the wide backward's partition and go to the reductions the wide head uses)."""
    b, nv, c = shape
    gs4 = torch.empty(b * nv, 4, dtype=torch.float32, device=grad_pos.device)
    rows = int(_lib.lib().geom_zn_gcn_bwd_partial_rows(b, nv, c, k, csr.ell_w))
    bg = _pass.bias_gradient(bias, c, grad_pos.device, (rows, c)) if want_bias else _pass.NO_BIAS_GRADIENT
    _lib.call("geom_zn_gcn_narrow_head_bwd_f32", b, nv, c, k, *_table(csr, True), grad_pos, float(scale), sign, act, gs4,
              bg.scratch)
    bg.finish(rows)
    return gs4, bg.out
