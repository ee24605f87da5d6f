"""Gradient work that a backward pass postpones to its end, and the one callback per pass that finishes it.

The layers (geometrics_amd.layers) may leave the partial sums of their bias and weight gradients (one reduction launch for
all layers instead of a launch-floor kernel per layer, with the step of `optim.FusedAdam.in_backward()` riding in it), the
weight-gradient products of equal layers (`layers.weight_gradient_batching()`: one batched product per run) and the input
gradient of a layer whose input is a leaf (`late_input_gradients()`) for the end of the pass.  Such a pass gets ONE record
(`_Pass`), created by its first job and finished by ONE end-of-pass callback of the engine (what DDP uses for its own
finalisation) in a fixed order: the reductions, the batched products, the `on_parameter_gradients` hooks, the postponed input
gradients.  A gradient handed to autograd is complete when backward() returns, not while the pass runs: a parameter that
something could read earlier (an existing .grad, a hook, a second live node feeding it) takes the immediate path, as does
every call outside an engine-run pass.  Deferral is OPT-IN (round-2 advice): C++ hooks on the AccumulateGrad node (DDP's
Reducer) and plain torch ops consuming a parameter cannot be seen from here.  bench.py and the deformation block's own
training step switch it on, nothing else does.

The switches are PROCESS-WIDE, not per thread: the backward nodes that read them run on the engine's device threads, not on
the thread that entered the context manager.
"""
import contextlib
import ctypes
import threading
import types
import weakref
from collections import namedtuple

import torch

from . import _lib
from . import dense as _dense_kernels
from ._identity import ByTensor


_DEFAULTS = {"defer": False,      # deferred_parameter_gradients(): bias / weight gradients finished at the end of the pass
             "late": False,       # late_input_gradients(): a leaf's input-gradient product postponed behind them
             "collect": None}     # late_input_gradients(collect=): where the postponed products go instead of being launched
switches = types.SimpleNamespace(
    ready_hooks=[],     # late_input_gradients(on_parameter_gradients): run once the parameter gradients are launched
    optimizer=None,     # optim.FusedAdam.in_backward(): its step rides in the end-of-pass reduction launch
    zero_fill=False,    # debugging aid: zero-filled placeholders (detect_anomaly trips over uninitialised memory)
    **_DEFAULTS)
_entered = []           # the settings of the switching contexts entered and not yet left, oldest first
_entered_lock = threading.Lock()


@contextlib.contextmanager
def _switched(**values):
    """`values` hold while the context is active.  Contexts entered on several threads may be left in any order: the switches
    are those of the latest entered context still active, the defaults once none is."""
    with _entered_lock:
        _entered.append(values)
        _apply()
    try:
        yield
    finally:
        with _entered_lock:
            del _entered[next(i for i, entry in enumerate(_entered) if entry is values)]
            _apply()


def _apply():
    current = dict(_DEFAULTS)
    for values in _entered:
        current.update(values)
    for name, value in current.items():
        setattr(switches, name, value)


def deferred_parameter_gradients(enabled=True):
    """Context manager: inside it, bias / weight gradients of a backward pass are finished by batched launches at the end
    of the pass (the caller guarantees that nothing reads a parameter gradient before backward() returns)."""
    return _switched(defer=enabled)


@contextlib.contextmanager
def late_input_gradients(on_parameter_gradients=None, enabled=True, collect=None):
    """Context manager around forward + backward of a data-parallel step (bench.py, N > 1): the gradient all-reduce waits
    only for the end-of-pass reduction launch, while the first layer's input gradient dX = G . W^T (65 us at the BASELINE
    shard) is needed by nobody before backward() returns.  It is postponed behind `on_parameter_gradients` (a callable run
    once every parameter gradient of the pass has been launched: where the step records the event its collective waits for),
    so that it runs while the all-reduce travels.  collect: a list -- the postponed products are NOT launched by the callback
    but appended to it as callables (each launches one product into the gradient buffer autograd already holds); the caller
    launches them, e.g. after issuing a collective.  They stay valid for as long as their tensors do (a captured step replays
    them every step)."""
    hooks = [on_parameter_gradients] if on_parameter_gradients is not None else []
    switches.ready_hooks.extend(hooks)
    try:
        with _switched(late=enabled, collect=collect):
            yield
    finally:
        for hook in hooks:
            switches.ready_hooks.remove(hook)


def set_optimizer(opt):
    """optim.FusedAdam.in_backward(): `opt` (None: none) steps inside the end-of-pass reduction launch when that launch
    finishes the gradient of every one of its parameters.  Returns the previous one."""
    prev, switches.optimizer = switches.optimizer, opt
    return prev


# ---- gradient targets (data-parallel steps: geometrics_amd.dist.GradBucket(bind=True)) ------------------------------------
# A parameter bound to a tensor of its shape gets its gradient WRITTEN THERE by the layers' launches: the end-of-pass reduction
# writes straight into the flat all-reduce bucket, autograd adopts the tensor as `.grad` (a fresh contiguous tensor object of
# the parameter's layout is taken as is), and the bucket's pack launch has nothing left to gather.
_gradient_targets = ByTensor(versioned=False)      # parameter (whatever the optimiser has done to it in place) -> its target


def bind_gradient_targets(params, tensors):
    """`tensors[i]` (same shape / dtype / device as `params[i]`, contiguous) receives the gradient of `params[i]` from now on;
    None unbinds.  Only gradients the layers produce themselves land there (a library-product fallback returns its own tensor)."""
    for p, t in zip(params, tensors):
        if t is None:
            _gradient_targets.drop(p)
            continue
        if t.shape != p.shape or t.dtype != p.dtype or t.device != p.device or not t.is_contiguous():
            raise ValueError("a gradient target must match its parameter's shape, dtype and device and be contiguous")
        _gradient_targets.put(t, p)


def _gradient_buffer(param, like):
    """Where the gradient of `param` (may be None: unknown) goes: its bound target, else a new tensor like `like`."""
    target = _gradient_targets.get(param) if param is not None else None
    # (a parameter that already holds a gradient is being ACCUMULATED into: the new gradient must not overwrite the old one's
    # memory, which is what the target is by then)
    # (a parameter fed by more than one live autograd node -- a shared weight or bias, a layer applied twice -- has its
    # gradients ADDED by the engine: each node needs memory of its own, or the second would overwrite the first's before the
    # sum is formed; GradBucket.pack() gathers a gradient that did not land in its view by copy)
    if target is not None and target.shape == like.shape and param.grad is None and _user_count(param) <= 1:
        return target.detach()           # a fresh tensor object over the target's memory (autograd adopts it as .grad)
    return torch.zeros_like(like) if switches.zero_fill else torch.empty_like(like)


# ---- parameter -> the live autograd nodes that produce a gradient for it: a parameter shared by two layers (or a layer applied
# twice) gets its gradients ADDED by the engine inside the pass, which reads them on arrival -- more than one live node means
# immediate reduction for all of them.  Nodes leave the set when their graph is freed.
_users = ByTensor(versioned=False)      # parameter -> WeakSet of nodes


def parameter_ref(param, node, needs_grad):
    """A weak reference to `param` (None for None) for the backward of `node`, which is registered as one of the parameter's
    live users when it produces a gradient for it."""
    if param is None:
        return None
    if needs_grad:
        nodes = _users.get(param)
        if nodes is None:
            nodes = _users.put(weakref.WeakSet(), param)
        nodes.add(node)
    return weakref.ref(param)


def _user_count(param):
    nodes = _users.get(param)
    return len(nodes) if nodes is not None else 0


def _alias(t):
    """A second tensor object over t's memory (no view relation): keeps the storage alive without being a reference to
    the tensor itself, so that autograd still finds the gradient unshared and stores it instead of cloning it."""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), t.storage_offset(), t.size(), t.stride())


def _engine_pass():      # inside an engine-run, first-order backward pass
    return (hasattr(torch._C, "_current_graph_task_id") and torch._C._current_graph_task_id() >= 0
            and not torch.is_grad_enabled())


def may_defer(param, opted_in=False):
    """Whether the gradient of `param` may be finished at the end of the pass.  opted_in: the forward ran inside
    weight_gradient_batching() -- that context is the caller's explicit request."""
    if not (switches.defer or opted_in) or param is None or not _engine_pass():
        return False
    if not param.is_leaf or _user_count(param) > 1:      # (another node of a live graph feeds the same parameter)
        return False
    return param.grad is None and not param._backward_hooks and not getattr(param, "_post_accumulate_grad_hooks", None)


def may_postpone_input_gradient(x):
    """A leaf whose gradient nobody observes before backward() returns: no tensor hooks (they would not see the postponed
    part), an engine-run first-order pass, deferral of the parameter gradients active (the flush this rides on).  The
    postponing node returns NO gradient for the leaf to the engine; the end-of-pass callback launches the product into a
    buffer of its own and then SETS the leaf's .grad to it -- or adds it to what other consumers of the leaf contributed
    through the engine (or an earlier pass left behind), so any number of consumers is correct (round-4 advice).  Only under
    .backward(): torch.autograd.grad(..., inputs=[leaf]) collects what the ENGINE carries and fails loudly ("not used in the
    graph") for such a leaf."""
    if not (switches.late and switches.defer) or not _engine_pass():
        return False
    return x.is_leaf and not x._backward_hooks and not getattr(x, "_post_accumulate_grad_hooks", None)


def _check_landed(param_ref, out):
    """After a deferred reduction: the gradient autograd stored for the parameter must BE the buffer the flush wrote.  If
    the engine kept a copy instead (it clones a gradient it does not hold the only reference to), the finished values are
    copied into it -- never leave a placeholder behind silently."""
    param = param_ref() if param_ref is not None else None
    if param is None or param.grad is None or param.grad.data_ptr() == out.data_ptr():
        return
    if param.grad.shape == out.shape or param.grad.numel() == out.numel():
        param.grad.copy_(out.view_as(param.grad))
    else:
        raise RuntimeError("geometrics_amd: a deferred parameter gradient did not reach its parameter (shape %s vs %s)"
                           % (tuple(param.grad.shape), tuple(out.shape)))


# ---- the jobs of a pass (param: a weak reference to the parameter whose gradient `out` is, or None) --------------------------
_Colsum = namedtuple("_Colsum", "partials rows cols out stream param")   # bias gradient: column sums of partials [rows, cols]
_Reduce = namedtuple("_Reduce", "rows cin c workspace out stream param")  # weight gradient: split partial sums -> out [cin, c]
# weight gradient out = x^T . g inside weight_gradient_batching(); launch_run(jobs) issues a list of them in layer order
_Product = namedtuple("_Product", "x g out stream param launch_run")
_Late = namedtuple("_Late", "launch out stream leaf")     # a leaf's input gradient: launch() writes it into out


class _Pass:
    """What one backward pass left for its end."""
    __slots__ = ("colsums", "reduces", "products", "late")

    def __init__(self):
        self.colsums, self.reduces, self.products, self.late = [], [], [], []

    def finish(self):
        # 1. the reductions
        colsums, reduces, self.colsums, self.reduces = self.colsums, self.reduces, [], []
        streams = {job.stream for job in colsums + reduces}
        if (reduces and colsums and len(streams) == 1 and all(job.cols % 4 == 0 for job in colsums)
                and 2 * len(reduces) + len(colsums) <= _lib.DENSE_MAX_REDUCE_JOBS):
            _launch_joint(reduces, colsums, streams.pop())
        else:
            _launch_colsums(colsums)
            _launch_reduces(reduces)
        # 2. the batched weight-gradient products, in layer order (the backward pass queued them in reverse): every operand
        # of a run of equal layers ascending
        products, self.products = self.products[::-1], []
        if products:
            products[0].launch_run(products)
        for job in reduces + colsums + products:
            _check_landed(job.param, job.out)
        # 3. every parameter gradient of the pass is launched
        for hook in list(switches.ready_hooks):
            hook()
        # 4. the postponed input-gradient products
        late, self.late, launches = self.late, [], []
        for job in late:
            launches.append(_on_stream(job.stream, job.launch))
            x = job.leaf()
            if x is not None and x.grad is None:
                x.grad = job.out.view(x.shape)           # the product's own buffer becomes the leaf's gradient: no copy
            elif x is not None:                          # other consumers of the leaf (or an earlier pass) were there first: add
                launches.append(_on_stream(job.stream, lambda x=x, out=job.out: x.grad.add_(out.view_as(x.grad))))
        if switches.collect is not None:
            switches.collect.extend(launches)
        else:
            for launch in launches:
                launch()


def _on_stream(stream, fn):
    def launch():
        with torch.cuda.stream(stream), torch.no_grad():
            fn()
    return launch


def _ints(seq):
    return (ctypes.c_int * len(seq))(*seq)


def _colsum_args(jobs):
    return (len(jobs), [j.partials for j in jobs], _ints([j.rows for j in jobs]), _ints([j.cols for j in jobs]),
            [j.out for j in jobs])


def _by_stream(jobs):
    groups = {}
    for job in jobs:
        groups.setdefault(job.stream, []).append(job)
    return groups.items()


def _launch_colsums(jobs):
    for stream, group in _by_stream(jobs):
        for c0 in range(0, len(group), _lib.COLSUM_MAX_JOBS):
            _lib.check(_lib.status("geom_colsum_batch_f32", *_colsum_args(group[c0:c0 + _lib.COLSUM_MAX_JOBS]),
                                   stream=stream.cuda_stream), "geom_colsum_batch_f32")


def _launch_reduces(jobs):
    for stream, group in _by_stream(jobs):
        _dense_kernels.reduce([(j.rows, j.cin, j.c, j.workspace, j.out, None) for j in group], stream.cuda_stream)


def _launch_joint(reduces, colsums, stream):
    """Weight AND bias gradients in one launch -- with the optimiser's step when the launch finishes the gradient of every one
    of its parameters."""
    weights = (len(reduces), _ints([j.rows for j in reduces]), _ints([j.cin for j in reduces]), _ints([j.c for j in reduces]),
               [j.workspace for j in reduces], [j.out for j in reduces])
    biases = _colsum_args(colsums)
    opt = switches.optimizer
    slots = None
    if opt is not None:
        index = {id(p): k for k, p in enumerate(opt.params)}
        slots = [index.get(id(job.param())) if job.param is not None else None for job in reduces + colsums]
        if None in slots or sorted(slots) != list(range(len(opt.params))) or opt.params[0].device != stream.device:
            slots = None
    if slots is None:
        _lib.check(_lib.status("geom_dense_reduce2_f32", *weights, None, *biases, stream=stream.cuda_stream),
                   "geom_dense_reduce2_f32")
    else:
        pick = lambda seq, ks: [seq[k] for k in ks]
        wk, bk = slots[:len(reduces)], slots[len(reduces):]
        params = [p.data for p in opt.params]
        _lib.check(_lib.status(
            "geom_dense_reduce_adam_f32",
            *weights, pick(params, wk), pick(opt.exp_avg, wk), pick(opt.exp_avg_sq, wk),
            *biases, pick(params, bk), pick(opt.exp_avg, bk), pick(opt.exp_avg_sq, bk), float(opt.lr), float(opt.betas[0]),
            float(opt.betas[1]), float(opt.eps), opt.state, stream=stream.cuda_stream), "geom_dense_reduce_adam_f32")
        opt._stepped_in_backward = True


# ---- the registry: autograd graph-task id -> the record of that pass ----------------------------------------------------------
_passes = {}
_passes_lock = threading.Lock()      # two passes may run at once, on two threads


def _current():
    """The record of the running pass; its first job creates it and queues its end-of-pass callback."""
    task = torch._C._current_graph_task_id()
    with _passes_lock:
        record = _passes.get(task)
        if record is not None:
            return record
        for stale in [t for t in _passes if t < task - 64]:      # passes that died of an exception never reach their callback
            del _passes[stale]
        record = _passes[task] = _Pass()
    torch.autograd.Variable._execution_engine.queue_callback(lambda: _finish(task, record))
    return record


def _finish(task, record):
    try:
        record.finish()
    finally:
        with _passes_lock:
            _passes.pop(task, None)


def pending(*kinds):
    """How many jobs of the given kinds ("colsums", "reduces", "products", "late"; all when none is named) wait in any pass."""
    with _passes_lock:
        return sum(len(getattr(record, kind)) for record in _passes.values() for kind in kinds or _Pass.__slots__)


# ---- what the layers' backward nodes call ---------------------------------------------------------------------------------
class BiasGradient(namedtuple("BiasGradient", "out scratch defer bias")):
    """The gradient of a [c] bias that a kernel leaves as per-workgroup partial column sums in `scratch`: `out` is what
    autograd gets (the bias's bound target or a new buffer); `defer`: the column sums wait for the end-of-pass launch."""
    __slots__ = ()

    @property
    def now(self):
        """Where a kernel that can finish the column sums itself writes them: None when they are deferred."""
        return None if self.defer else self.out

    def finish(self, rows):
        """After a kernel that left only the [rows, c] partials: their column sums are queued, or launched now."""
        if self.out is None:
            return
        stream = torch.cuda.current_stream(self.out.device)
        if self.defer:      # (only a live leaf bias is deferred)
            _current().colsums.append(_Colsum(self.scratch, rows, self.out.shape[0], _alias(self.out), stream, weakref.ref(self.bias)))
        else:
            _launch_colsums([_Colsum(self.scratch, rows, self.out.shape[0], self.out, stream, None)])


NO_BIAS_GRADIENT = BiasGradient(None, None, False, None)


def bias_gradient(bias, c, device, scratch_shape, opted_in=False):
    """The buffer, the partial-sum scratch and the defer decision of a bias gradient (bias may be None: unknown)."""
    out = _gradient_buffer(bias, bias) if bias is not None and bias.shape == (c,) and bias.dtype == torch.float32 \
        else torch.empty(c, dtype=torch.float32, device=device)
    scratch = torch.empty(scratch_shape, dtype=torch.float32, device=device)
    return BiasGradient(out, scratch, may_defer(bias, opted_in), bias)


def weight_gradient(param_ref, w, rows, cin, c, workspace):
    """The weight gradient whose split partial sums are in `workspace`: queued for the reduction launch at the end of the
    pass where deferral is allowed (its buffer handed to autograd now), reduced at once otherwise."""
    param = param_ref()
    out = _gradient_buffer(param, w)
    if may_defer(param):
        stream = torch.cuda.current_stream(w.device)
        _current().reduces.append(_Reduce(rows, cin, c, workspace, _alias(out).view(cin, c), stream, param_ref))
    else:
        _dense_kernels.reduce([(rows, cin, c, workspace, out.view(cin, c), None)])
    return out


def postpone_weight_product(x, g, out, param_ref, launch_run):
    """out = x^T . g, issued at the end of the pass with the pass's other such products by `launch_run`."""
    _current().products.append(_Product(x, g, _alias(out).view(x.shape[1], g.shape[1]), torch.cuda.current_stream(out.device),
                                        param_ref, launch_run))


def postpone_input_gradient(launch, out, leaf):
    """`launch()` writes the input gradient of `leaf` into `out` behind everything else of the pass (see above)."""
    _current().late.append(_Late(launch, out, torch.cuda.current_stream(out.device), weakref.ref(leaf)))
