"""Adam for the replicated 0N-GCN parameters with the interface of torch.optim.Adam: zero_grad / step / param_groups /
state_dict / load_state_dict.  Same update as torch.optim.Adam(lr, betas, eps) without weight decay / amsgrad (what
GEOMetrics.py:73 uses); the step counter and the beta powers live on the device and are advanced inside the kernel (HIP-graph
replayable, no tick launch).  Two routes, same bits:

  chunked  geom_adam_step_f32, up to 64 parameter tensors per launch.  More tensors are issued in chunks of 64 that all use the
           bias corrections of the same step -- only the last chunk advances the state.  `lr` is a by-value kernel argument: a
           captured step replays with the lr it was captured with.
  table    geom_adam_table_step_f32, ONE launch for any number of tensors: the per-tensor records live in a device table and
           `lr` in a device array with one entry per parameter group.  Only this route follows an lr change under replay:
           change `param_groups[i]['lr']`, call `sync_hyperparameters()`, and the next replay uses it with no re-capture.

The table route is taken with `table=True` (or GEOM_ADAM_TABLE=1 in the environment), and whenever the chunked route would need
more than one launch; `table=False` keeps the chunked route for any tensor count.  For the cases one chunked launch serves it is
OFF by default: not measured against that launch yet (tools/time_adam.py).

Parameter groups may differ in `lr` only: the device state holds ONE pair of beta powers, so betas and eps are shared.
Parameters that do not require a gradient are dropped from their group (indices in state_dict() count the kept ones)."""
import ctypes
import os

import numpy as np
import torch

from . import _lib, backward_pass

_BLOCK = 1024       # elements per workgroup: 256 threads x 4 (csrc/adam.hip)
_SPARES = 16        # pinned table buffers kept ready for captures (nothing is allocated while one runs)


def beta_power(beta, t):
    """beta^t as the kernel's step state holds it after t steps: float32, `beta` for t = 1, then one multiply per step
    (adam_math.h: b1t = st[1] * b1).  NOT beta ** t, which differs in the last bits.  0.0 for t = 0 (the kernel never reads
    it then).  The chain ends in a fixed point -- 0 for beta < 0.5, else the subnormal that beta no longer rounds down (the
    kernels keep float32 subnormals: 7e-43 for 0.999, reached after ~97 000 steps) -- and the loop stops there."""
    t = int(t)
    if t <= 0:
        return np.float32(0.0)
    b = np.float32(beta)
    power, left = b, t - 1
    while left > 0 and np.float32(power * b) != power:
        n = min(left, 1 << 16)
        chain = np.full(n + 1, b, dtype=np.float32)
        chain[0] = power
        power = np.multiply.accumulate(chain)[-1]       # sequential: ((power * b) * b) * ...
        left -= n
    return np.float32(power)


class _InBackward:
    def __init__(self, opt):
        self.opt = opt

    def __enter__(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError("FusedAdam.in_backward() would step on the LOCAL gradients, before the all-reduce across the "
                               "%d ranks; data-parallel steps call step(bucket.views, grad_scale=1/world) after the exchange"
                               % dist.get_world_size())
        # the end-of-pass launch takes ONE lr (opt.lr): groups whose lr differ leave the step to step()
        self.prev = backward_pass.set_optimizer(self.opt if self.opt._one_lr() else None)
        self.opt._stepped_in_backward = False
        return self.opt

    def __exit__(self, *exc):
        backward_pass.set_optimizer(self.prev)
        return False


class _Table:
    """One device table + the pinned host buffer it was copied from + what they hold."""
    def __init__(self, host, dev):
        self.host, self.dev = host, dev
        self.key = None
        self.blocks = 0
        self.captured = False       # a HIP-graph capture recorded a copy from `host` or a launch that reads `dev`


class FusedAdam:
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, table=None):
        """params: parameter tensors, or torch.optim-style group dicts ({'params': [...], 'lr': ...}).
        table: True / False = the table / the chunked route always; None = the table route when GEOM_ADAM_TABLE=1 or when
        the chunked route would need more than one launch."""
        params = list(params)
        groups = params if params and isinstance(params[0], dict) else [{"params": params}]
        defaults = {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay, "amsgrad": amsgrad}
        self.param_groups = []
        for g in groups:
            g = dict(defaults, **g)
            ps = g["params"]
            g["params"] = [p for p in ([ps] if isinstance(ps, torch.Tensor) else ps) if p.requires_grad]
            g["betas"] = tuple(g["betas"])
            self.param_groups.append(g)
        self._check_groups(self.param_groups)
        self.params = [p for g in self.param_groups for p in g["params"]]
        if not self.params:
            raise RuntimeError("FusedAdam got no trainable parameters")
        if len(set(map(id, self.params))) != len(self.params):
            raise ValueError("FusedAdam: a parameter appears in more than one group")
        for p in self.params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("FusedAdam needs contiguous fp32 parameters on a HIP device")
        self.table = (os.environ.get("GEOM_ADAM_TABLE", "0") not in ("", "0") or None) if table is None else bool(table)
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.state = torch.zeros(_lib.ADAM_STATE_WORDS, dtype=torch.float32, device=self.params[0].device)
        self._stepped = [False] * len(self.params)      # host-side: has this parameter ever been stepped (state_dict())
        self._group_of = [k for k, g in enumerate(self.param_groups) for _ in g["params"]]
        self._lr_dev = torch.zeros(len(self.param_groups), dtype=torch.float32, device=self.params[0].device)
        self._lr_sent = None        # the values _lr_dev holds
        self._tab = None            # the current _Table
        self._tabs_kept = []        # tables a captured graph reads: never rewritten, alive as long as the optimiser
        self._spare_hosts = []      # pinned buffers set aside (by an eager step) for tables that change inside a capture

    # ---- hyper-parameters ------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_groups(groups):
        for g in groups:
            if g["weight_decay"] != 0 or g["amsgrad"]:
                raise ValueError("FusedAdam implements torch.optim.Adam without weight decay and without amsgrad (got "
                                 "weight_decay=%r, amsgrad=%r)" % (g["weight_decay"], g["amsgrad"]))
            if tuple(g["betas"]) != tuple(groups[0]["betas"]) or g["eps"] != groups[0]["eps"]:
                raise ValueError("FusedAdam keeps ONE pair of beta powers on the device: every parameter group must have the "
                                 "same betas and eps (only lr may differ)")

    @property
    def lr(self):
        """Group 0's learning rate (what the in-backward step reads)."""
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, value):
        self.param_groups[0]["lr"] = value

    @property
    def betas(self):
        return self.param_groups[0]["betas"]

    @property
    def eps(self):
        return self.param_groups[0]["eps"]

    def _one_lr(self):
        return all(float(g["lr"]) == float(self.lr) for g in self.param_groups)

    def sync_hyperparameters(self):
        """Bring the device-side lr array up to `param_groups` (a non-blocking copy, only when a value changed).  Every eager
        step() does this itself; a loop that REPLAYS a captured step calls it after changing an lr, and the next replay of the
        table route uses the new value.  (The chunked route's lr is a launch argument: it needs a re-capture.)"""
        self._check_groups(self.param_groups)
        lrs = [float(g["lr"]) for g in self.param_groups]
        if lrs == self._lr_sent:
            return
        if torch.cuda.is_current_stream_capturing():
            # a copy recorded here would be replayed every step and overwrite what a later sync_hyperparameters() wrote
            raise RuntimeError("FusedAdam: the device's learning rates are not those of param_groups; call "
                               "sync_hyperparameters() (or run the eager warm-up step) before the capture, not inside it")
        self._lr_dev.copy_(torch.tensor(lrs, dtype=torch.float32).pin_memory(), non_blocking=True)
        self._lr_sent = lrs

    # ---- the step ----------------------------------------------------------------------------------------------------------
    @property
    def step_count(self):
        """Steps taken so far (one host read)."""
        return int(self.state[0].item())

    def in_backward(self):
        """Context manager around forward + backward of ONE iteration: the step is applied INSIDE the backward pass, in the
        launch that finishes the gradients (the end-of-pass reduction, geom_dense_reduce_adam_f32) -- no optimiser
        launch of its own, no second read of the gradients.  It happens only if (a) parameter-gradient deferral is on
        (`layers.deferred_parameter_gradients()`) and (b) that one launch finishes the gradient of EVERY parameter of this
        optimiser, each exactly once; the following `step()` (no arguments, grad_scale 1) is then a no-op.  Otherwise
        nothing changes and `step()` does the work.  For `zero_grad(); backward(); step()` loops -- not for gradient
        accumulation over several passes, and not for data-parallel steps (they reduce the gradients across ranks between
        backward and step).  Parameter groups whose lr differ: the launch takes one lr, so `step()` does the work."""
        return _InBackward(self)

    def _consume_in_backward(self):
        if getattr(self, "_stepped_in_backward", False):    # that launch stepped EVERY parameter
            self._stepped = [True] * len(self.params)
        self._stepped_in_backward = False

    def zero_grad(self, set_to_none=True):
        self._consume_in_backward()     # a new iteration: an in-backward step nobody consumed must not swallow a later step()
        for p in self.params:
            p.grad = None

    def step(self, grads=None, grad_scale=1.0):
        """grads: tensors to read instead of p.grad (e.g. views of an all-reduced flat bucket).  A parameter whose
        gradient is None is left untouched, as torch.optim.Adam does (the reference block's bn14 is never used)."""
        if grads is None:
            if getattr(self, "_stepped_in_backward", False) and grad_scale == 1.0:
                self._consume_in_backward()             # the backward pass's reduction launch has applied this step
                return
        if getattr(self, "_stepped_in_backward", False):
            # the pass already applied a step with the parameters' own gradients and scale 1: a second, different step on top
            # of it is never what the caller meant
            self._consume_in_backward()
            raise RuntimeError("FusedAdam.step(grads=..., grad_scale=...) after a backward pass that already applied the step "
                               "(in_backward()): this iteration would be stepped twice")
        if grads is None:
            grads = [p.grad for p in self.params]
        live = [i for i, g in enumerate(grads) if g is not None]
        stepped = live
        live = [i for i in live if self.params[i].numel()]      # an empty tensor has no address to hand over, nothing to update
        if not live:
            return
        grads = [None if g is None else g.contiguous() for g in grads]
        # chunks of the chunked route: at most 64 tensors, one lr each
        m = _lib.ADAM_MAX_TENSORS
        chunks = []
        for i in live:
            lr = float(self.param_groups[self._group_of[i]]["lr"])
            if chunks and len(chunks[-1][1]) < m and chunks[-1][0] == lr:
                chunks[-1][1].append(i)
            else:
                chunks.append((lr, [i]))
        with torch.cuda.device(self.params[0].device):      # (the table step asks about capture and copies on the current stream)
            if self.table or (self.table is None and len(chunks) > 1):
                self._table_step(live, grads, grad_scale)
            else:
                self._check_groups(self.param_groups)
                for k, (lr, chunk) in enumerate(chunks):
                    pick = lambda seq: [seq[i] for i in chunk]
                    sizes = (ctypes.c_int64 * len(chunk))(*[self.params[i].numel() for i in chunk])
                    _lib.call("geom_adam_step_f32", len(chunk), pick([p.data for p in self.params]), pick(grads),
                              pick(self.exp_avg), pick(self.exp_avg_sq), sizes, lr, float(self.betas[0]), float(self.betas[1]),
                              float(self.eps), float(grad_scale), self.state,
                              int(k + 1 == len(chunks)))      # only the last chunk advances the device-side step state
        for i in stepped:
            self._stepped[i] = True

    def _table_step(self, live, grads, grad_scale):
        """ONE launch for all live tensors.  The table goes to the device only when a pointer, a size or a group differs from
        what the device holds: eager steps get a fresh p.grad after zero_grad() and re-upload; bucket views and captured
        steps have stable pointers and do not."""
        capturing = torch.cuda.is_current_stream_capturing()
        self.sync_hyperparameters()
        n = len(live)
        cols = np.empty((5, n), dtype=np.int64)
        cols[0] = [self.params[i].data_ptr() for i in live]
        cols[1] = [grads[i].data_ptr() for i in live]
        cols[2] = [self.exp_avg[i].data_ptr() for i in live]
        cols[3] = [self.exp_avg_sq[i].data_ptr() for i in live]
        cols[4] = [self.params[i].numel() for i in live]
        group = np.array([self._group_of[i] for i in live], dtype=np.int32)
        key = cols.tobytes() + group.tobytes()
        words = 6 * len(self.params)        # room for every parameter (geom_adam_table_bytes / 8), whatever is live
        while not capturing and len(self._spare_hosts) < _SPARES:
            self._spare_hosts.append(torch.empty(words, dtype=torch.int64, pin_memory=True))
        tab = self._tab
        if tab is None or tab.key != key:
            # A table a capture has recorded is never rewritten: a replay must not read a half-written or a later table.  A
            # table only eager steps used gets a fresh pinned buffer all the same -- the copy out of the old one may still
            # be in flight; torch's pinned allocator takes the old one back once that copy has completed.  Nothing is
            # allocated or released while a capture runs: it takes the buffers an earlier eager step set aside (one per
            # step() of the capture whose gradients moved).
            if capturing:
                if not self._spare_hosts:
                    raise RuntimeError("FusedAdam: the table changed inside a capture and no pinned buffer is left of the %d an "
                                       "eager step() sets aside; run one eager step() (the warm-up) before every capture, and "
                                       "capture at most %d steps into one graph" % (_SPARES, _SPARES))
                host = self._spare_hosts.pop()
            else:
                host = torch.empty(words, dtype=torch.int64, pin_memory=True)
            if tab is not None and (tab.captured or capturing):
                self._tabs_kept.append(tab)
            dev = tab.dev if tab is not None and not tab.captured else torch.empty(words, dtype=torch.int64,
                                                                                   device=self.state.device)
            tab = self._tab = _Table(host, dev)  # stream order keeps the launches that read dev's old contents ahead of the copy
            blocks = (cols[4] + (_BLOCK - 1)) // _BLOCK
            tab.blocks = int(blocks.sum())
            size = _lib.lib().geom_adam_table_bytes(n, tab.blocks)
            if size < 0:
                _lib.check(int(size), "geom_adam_table_bytes")
            view = host.numpy()[:size // 8]
            view[:5 * n] = cols.reshape(-1)
            tail = view[5 * n:].view(np.int32)
            tail[:n] = np.cumsum(blocks) - blocks       # first_block
            tail[n:] = group
            tab.dev.copy_(host, non_blocking=True)
            tab.key = key
        tab.captured = tab.captured or capturing
        _lib.call("geom_adam_table_step_f32", n, tab.dev, tab.blocks, self._lr_dev, float(self.betas[0]), float(self.betas[1]),
                  float(self.eps), float(grad_scale), self.state, 1)

    # ---- checkpoints -------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim.Adam's layout: state[i] = {'step' (0-dim float32 CPU tensor), 'exp_avg', 'exp_avg_sq'} for every
        parameter stepped at least once (a parameter that never had a gradient is absent, as in torch), param_groups with
        `params` as indices -- torch.optim.Adam.load_state_dict takes it.  One extra top-level key, 'geom_step_state': the
        device's {t, beta1^t, beta2^t} as three floats (torch ignores it).  One host read; the moments are references, as
        in torch."""
        self._consume_in_backward()
        t, b1t, b2t = self.state[:3].tolist()
        state = {i: {"step": torch.tensor(t, dtype=torch.float32), "exp_avg": self.exp_avg[i],
                     "exp_avg_sq": self.exp_avg_sq[i]} for i in range(len(self.params)) if self._stepped[i]}
        groups, at = [], 0
        for g in self.param_groups:
            packed = {k: v for k, v in g.items() if k != "params"}
            packed["params"] = list(range(at, at + len(g["params"])))
            at += len(g["params"])
            groups.append(packed)
        return {"state": state, "param_groups": groups, "geom_step_state": [t, b1t, b2t]}

    def load_state_dict(self, sd):
        """Takes this optimiser's own dicts and plain torch.optim.Adam dicts with the same group structure.  Everything is
        checked before anything is modified (ValueError).  Without 'geom_step_state' the step count comes from the 'step'
        entries -- all equal: there is one step counter for all tensors -- and the beta powers are rebuilt by the kernel's
        own float32 recurrence (`beta_power`), so a resumed run equals the uninterrupted one bit for bit."""
        groups = [dict(g) for g in sd["param_groups"]]
        if len(groups) != len(self.param_groups):
            raise ValueError("FusedAdam.load_state_dict: %d parameter groups, this optimiser has %d"
                             % (len(groups), len(self.param_groups)))
        at = 0
        for g, mine in zip(groups, self.param_groups):
            if len(g["params"]) != len(mine["params"]) or list(g["params"]) != list(range(at, at + len(mine["params"]))):
                raise ValueError("FusedAdam.load_state_dict: a group of %d parameters where this optimiser has %d (parameters "
                                 "that do not require a gradient are not counted)" % (len(g["params"]), len(mine["params"])))
            at += len(mine["params"])
            g.setdefault("weight_decay", 0)
            g.setdefault("amsgrad", False)
            g["betas"] = tuple(g["betas"])
        self._check_groups(groups)
        state = sd["state"]
        for i, s in state.items():
            if not (isinstance(i, int) and 0 <= i < len(self.params)):
                raise ValueError("FusedAdam.load_state_dict: state of parameter %r, this optimiser has %d" % (i, len(self.params)))
            for name in ("exp_avg", "exp_avg_sq"):
                if tuple(s[name].shape) != tuple(self.params[i].shape):
                    raise ValueError("FusedAdam.load_state_dict: %s of parameter %d has shape %s, the parameter %s"
                                     % (name, i, tuple(s[name].shape), tuple(self.params[i].shape)))
        if sd.get("geom_step_state") is not None:
            words = [float(x) for x in sd["geom_step_state"]]
            if len(words) != 3:
                raise ValueError("FusedAdam.load_state_dict: geom_step_state is {t, beta1^t, beta2^t}")
        else:
            steps = {float(s["step"]) for s in state.values()}
            if len(steps) > 1:
                raise ValueError("FusedAdam.load_state_dict: the parameters' step counts differ (%s); this optimiser keeps "
                                 "one step counter for all tensors" % sorted(steps))
            t = steps.pop() if steps else 0.0
            if t < 0 or t != int(t):
                raise ValueError("FusedAdam.load_state_dict: step count %r" % t)
            b1, b2 = groups[0]["betas"]
            words = [t, float(beta_power(b1, t)), float(beta_power(b2, t))]
        # checked: modify
        self._consume_in_backward()
        for g, mine in zip(groups, self.param_groups):
            mine.update({k: v for k, v in g.items() if k != "params"})
        with torch.no_grad():
            for i in range(len(self.params)):
                s = state.get(i)
                self._stepped[i] = s is not None
                if s is None:
                    self.exp_avg[i].zero_()
                    self.exp_avg_sq[i].zero_()
                else:
                    self.exp_avg[i].copy_(s["exp_avg"])
                    self.exp_avg_sq[i].copy_(s["exp_avg_sq"])
            fresh = torch.zeros(_lib.ADAM_STATE_WORDS, dtype=torch.float32)      # the arrival counters re-armed
            fresh[:3] = torch.tensor(words, dtype=torch.float32)
            self.state.copy_(fresh)


def overlay_namespace():
    """What overlay/utils.py exports as `optim` under GEOM_OVERLAY_ADAM=fused: torch.optim, except that `Adam` builds a
    FusedAdam (torch's defaults; lr, betas and eps passed through; weight_decay != 0 / amsgrad raise ValueError)."""
    import types

    class _Optim(types.ModuleType):
        def __getattr__(self, name):
            return getattr(torch.optim, name)

    def Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        return FusedAdam(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)

    ns = _Optim("geometrics_amd.optim.overlay")
    ns.__doc__ = overlay_namespace.__doc__
    ns.__file__ = __file__
    ns.Adam = Adam
    return ns
