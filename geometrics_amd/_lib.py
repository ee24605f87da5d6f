"""ctypes binding of libgeom_hip.so (the C ABI declared in include/geom_hip.h).

torch is used only for device memory and the current HIP stream; the signatures, argument structs and limits are read
from the header (_header.py).  call() / status() / args() take tensors for the pointers and check them against the pointee
types declared there; lib() is the plain binding (every pointer untyped).  Loading fails loudly -- there is no fallback
implementation.
"""
import ctypes
import os

import torch

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgeom_hip.so")

# the limits, flags and codes of the header under the names the operators use (GEOM_X -> X)
_C = _header.CONSTANTS
ABI_VERSION = _C["ABI_VERSION"]
EUNSUPPORTED = _C["EUNSUPPORTED"]
FLAG_REF_TAIL_TRUNC = _C["FLAG_REF_TAIL_TRUNC"]
FLAG_FIX_REGION6 = _C["FLAG_FIX_REGION6"]
FLAG_TRI_BRUTE_FORCE = _C["FLAG_TRI_BRUTE_FORCE"]
FLAG_NN_FMA = _C["FLAG_NN_FMA"]
FLAG_TRI_WS_READY = _C["FLAG_TRI_WS_READY"]
FLAG_NN_SAMPLES_ONLY = _C["FLAG_NN_SAMPLES_ONLY"]
ADAM_MAX_TENSORS = _C["ADAM_MAX_TENSORS"]
ADAM_STATE_WORDS = _C["ADAM_STATE_WORDS"]
COLSUM_MAX_JOBS = _C["COLSUM_MAX_JOBS"]
DENSE_MAX_LAYERS = _C["DENSE_MAX_LAYERS"]
DENSE_MAX_REDUCE_JOBS = _C["DENSE_MAX_REDUCE_JOBS"]
SUM_MAX_TENSORS = _C["SUM_MAX_TENSORS"]
DEFORM_CHAIN_MAX = _C["DEFORM_CHAIN_MAX"]
DEFORM_TAIL = _C["DEFORM_TAIL"]
DEFORM_WIDE_MAX_B = _C["DEFORM_WIDE_MAX_B"]

# the argument structs, fields as the header orders them
DeformFwd = _header.STRUCTS["geom_deform_fwd"]
DeformBwd = _header.STRUCTS["geom_deform_bwd"]
DeformInfer = _header.STRUCTS["geom_deform_infer"]
DeformPlainFwd = _header.STRUCTS["geom_deform_plain_fwd"]
DeformPlainBwd = _header.STRUCTS["geom_deform_plain_bwd"]
SurfaceCull = _header.STRUCTS["geom_surface_cull"]
SurfaceTail = _header.STRUCTS["geom_surface_tail"]
FaceSplit = _header.STRUCTS["geom_face_split"]

# ---- package-wide reference-quirk mode (SURVEY quirk register Q1 / Q3) ------------------------------------------------
# The shipped CUDA kernels drop the tail of every 512-wide tile of targets / triangles (chamfer_distance.cu:31-33,
# tri_distance.cu:129,134); the default here is the full scan (= the reference's CPU nnsearch and its legacy kernels).
# With the mode on, every call that does not pass flags of its own -- ChamferDistance(), TriDistance(), chamfer_nn(),
# tri_distance(), batch_point_to_point / _surface, the compiled forward_cuda entry points -- reproduces the truncation
# exactly (GEOM_FLAG_REF_TAIL_TRUNC): what an unmodified driver needs to re-obtain the numbers of the reference's CUDA
# build, e.g. its validation F1 at 2466 points (GEOMetrics.py:227,349), where the last 2 targets are never seen.
_reference_quirks = os.environ.get("GEOM_REF_QUIRKS", "0") not in ("", "0")


def set_reference_quirks(on=True):
    """Switch the package-wide reference-quirk mode (initial value: environment variable GEOM_REF_QUIRKS)."""
    global _reference_quirks
    _reference_quirks = bool(on)
    from . import _shim
    if _shim._module is not None:          # the compiled entry points keep their own copy of the switch
        _shim._module.set_reference_quirks(_reference_quirks)
    return _reference_quirks


def reference_quirks():
    return _reference_quirks


def quirk_flags():
    """Flags of a call that passes none: GEOM_FLAG_REF_TAIL_TRUNC in reference-quirk mode, else 0."""
    return FLAG_REF_TAIL_TRUNC if _reference_quirks else 0


# ---- what may stand for a pointer of the ABI ---------------------------------------------------------------------------------
# None (NULL); a python int or a ctypes object (a host pointer, address arithmetic: passed on unchecked); a torch.Tensor -- on a
# HIP device, of a dtype the pointee declared in the header admits, on the device of every other tensor of the call; for a
# struct pointer an instance of that struct (args() below) or a list of them (a host array); for a `type *const *` a list /
# tuple of tensors and None.  Contiguity and shape are NOT looked at here (column views with a leading-dimension argument are
# legitimate): require() and the wrappers do that.  The smallest table that admits what the package passes:
ADMITS = {"float": (torch.float32,), "int": (torch.int32,), "int64_t": (torch.int64,),
          "uint16_t": (torch.int16,),      # sign masks, bf16 planes
          "uint64_t": (torch.int64,),      # the sampler state
          "void": None}                    # any dtype
# entry point / struct -> (number of arguments, [(position, name, C type, depth, admitted dtypes, struct class)] of its pointers)
_plans = {}


def _plan(name):
    """What to do with each pointer parameter of `name`, worked out from the header's table the first time `name` is called."""
    described = list(_header.PARAMETERS[name])
    if name in _header.PROTOTYPES and (not described or described.pop()[1:] != ("void", 1)):      # status() supplies the stream
        raise RuntimeError("%s takes no stream: call it on lib() directly" % name)
    pointers = []
    for i, (param, pointee, depth) in enumerate(described):
        struct = _header.STRUCTS.get(pointee)
        if depth and struct is None and pointee not in ADMITS:
            raise RuntimeError("%s: no tensor dtype is known for `%s %s%s`" % (name, pointee, "*" * depth, param))
        if depth:
            pointers.append((i, param, "%s %s" % (pointee, "*" * depth), depth, None if struct else ADMITS[pointee], struct))
    _plans[name] = plan = (len(described), pointers)
    return plan


def _address(name, p, t, dev):
    """data_ptr() of tensor `t` given for pointer `p` of `name` after the checks above -> (address, the call's device)."""
    why = None
    if not t.is_cuda:
        why = "it must live on a HIP device"
    elif p[4] is not None and t.dtype not in p[4]:
        why = "it must be %s" % " or ".join(map(str, p[4]))
    elif dev is not None and t.device != dev:
        why = "the call's other tensors are on %s" % dev
    if why:
        raise RuntimeError("%s: parameter `%s` (declared `%s%s`) was given a %s tensor on %s -- %s"
                           % (name, p[1], p[2], p[1], t.dtype, t.device, why))
    return t.data_ptr(), t.device


def _struct_device(name, p, a, dev):
    """Struct `a` given for pointer `p` of `name`: of the declared type, its tensors (args() below) on the call's device."""
    if type(a) is not p[5]:
        raise RuntimeError("%s: parameter `%s` (declared `%s%s`) was given a %s" % (name, p[1], p[2], p[1], type(a).__name__))
    on = a.__dict__.get("_device")
    if on is not None and dev is not None and on != dev:
        raise RuntimeError("%s: the tensors of `%s` are on %s, the call's other tensors on %s" % (name, p[1], on, dev))
    return on if dev is None else dev


def convert(name, values):
    """The C arguments of entry point (or the field values of struct) `name` from `values` under the rule above, and the
    device of the tensors among them (None: there were none).  Eager steps are host-bound: one test per tensor on the way
    through, _address() to say what was wrong."""
    count, pointers = _plans.get(name) or _plan(name)
    if len(values) != count:
        raise RuntimeError("%s takes %d arguments%s (%d given)" % (name, count, " and the stream" if name in _header.PROTOTYPES
                                                                    else "", len(values)))
    out, dev = list(values), None
    for p in pointers:
        a = out[p[0]]
        if a is None or type(a) is int:
            continue
        if isinstance(a, torch.Tensor):
            d = a.device
            if (d == dev or (dev is None and a.is_cuda)) and p[3] == 1 and (p[4] is None or a.dtype in p[4]):
                out[p[0]], dev = a.data_ptr(), d
            elif p[3] != 1:
                raise RuntimeError("%s: parameter `%s` (declared `%s%s`) takes a list of tensors" % (name, p[1], p[2], p[1]))
            else:
                out[p[0]], dev = _address(name, p, a, dev)
        elif isinstance(a, (list, tuple)):
            if p[5] is not None:          # a host array of argument structs
                out[p[0]] = array = (p[5] * len(a))()
                for j, s in enumerate(a):
                    dev = _struct_device(name, p, s, dev)
                    array[j] = s
            elif p[3] == 2:
                out[p[0]] = array = (ctypes.c_void_p * len(a))()
                for j, t in enumerate(a):
                    if t is not None:
                        array[j], dev = _address(name, p, t, dev)
            else:
                raise RuntimeError("%s: parameter `%s` (declared `%s%s`) takes no list" % (name, p[1], p[2], p[1]))
        elif isinstance(a, ctypes.Structure):
            dev = _struct_device(name, p, a, dev)
            out[p[0]] = ctypes.byref(a)
    return out, dev


def args(struct, *values):
    """An argument struct of the header from its field values in header order, pointers under the same rule.  The struct
    remembers the device of its tensors for the call it goes into; the tensors are the caller's to keep until the launch is
    issued."""
    cvalues, dev = convert(struct.__name__, values)
    a = struct(*cvalues)
    a._device = dev
    return a


def status(name, *args, stream=None):
    """Invoke an entry point on the device of its tensor arguments (the current one when it has none), on that device's current
    stream (or on `stream`, a raw hipStream_t), and return its code: 0, a hipError_t or a negative GEOM_E* -- for callers that
    look at GEOM_EUNSUPPORTED before they check()."""
    cargs, dev = convert(name, args)
    fn = getattr(lib(), name)
    if dev is not None and dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            return fn(*cargs, stream_ptr() if stream is None else stream)
    return fn(*cargs, stream_ptr() if stream is None else stream)


def call(name, *args):
    """Invoke an entry point as status() does and raise on failure."""
    check(status(name, *args), name)


def ptr(t):
    return None if t is None else t.data_ptr()

_lib = None


def _refuse_stale_library():
    """A library built from OTHER kernel sources than the ones on disk (an edit or a checkout without a rebuild) would run
    silently -- wrong numbers in every profile taken with it.  The build stamps the library with the digest of its sources;
    a mismatch is an error (GEOM_ALLOW_STALE_LIB=1 to load it anyway).  No stamp or no sources on disk: nothing to compare."""
    if os.environ.get("GEOM_ALLOW_STALE_LIB"):
        return
    try:
        from . import build
        built = build.built_digest()
        current = build.source_digest() if built else None
    except Exception:        # an installation without the sources
        return
    if built and current and built != current:
        raise RuntimeError("geometrics_amd: %s was built from other kernel sources than the ones on disk -- rebuild it with "
                           "`python -m geometrics_amd.build` (or set GEOM_ALLOW_STALE_LIB=1)" % LIB_PATH)


def lib():
    """The loaded library; raises RuntimeError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "geometrics_amd: %s is missing -- build it with `python -m geometrics_amd.build` "
                "(hipcc, gfx950). There is no CPU/PyTorch fallback." % LIB_PATH)
        _refuse_stale_library()
        # GEOM_LIB_OVERRIDE: an instrumented build of the same sources (tools/probe: tile stamps, counters) -- never the product.
        # Said loudly: a variable that leaks into a training environment would put a probe build behind production calls.
        override = os.environ.get("GEOM_LIB_OVERRIDE")
        if override:
            import sys
            print("geometrics_amd: GEOM_LIB_OVERRIDE is set -- loading %s instead of the product library (probe builds only; "
                  "its ABI version is checked, its sources are not)" % override, file=sys.stderr)
        L = ctypes.CDLL(override or LIB_PATH)
        if L.geom_abi_version() != ABI_VERSION:       # a stale library, before any of its symbols is looked up
            raise RuntimeError("geometrics_amd: libgeom_hip.so ABI %d != binding ABI %d; rebuild"
                               % (L.geom_abi_version(), ABI_VERSION))
        for name, (restype, argtypes) in _header.PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def declared_symbols():
    return sorted(_header.PROTOTYPES)


def check(code, what):
    if code != 0:
        msg = lib().geom_strerror(code).decode()
        raise RuntimeError("%s failed: %s (code %d)" % (what, msg, code))


def clear_hip_error():
    """Fetch-and-reset HIP's sticky last-error (e.g. after an aborted graph capture), so that the next
    launch check reports only its own failure.  Returns the stale code."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        return 0
    hip.hipGetLastError.restype = ctypes.c_int
    return hip.hipGetLastError()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def require(t, name, dtype, ndim=None, last=None):
    """Validate what the reference leaves unchecked (chamfer_distance.cpp:15-27): device, dtype,
    layout.  Returns a contiguous tensor (the reference wrappers call .contiguous() too)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must live on a HIP device (got %s); geometrics_amd has no CPU path"
                           % (name, t.device))
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError("%s must be %d-dimensional (got shape %s)" % (name, ndim, tuple(t.shape)))
    if last is not None and t.shape[-1] != last:
        raise RuntimeError("%s must have last dimension %d (got shape %s)" % (name, last, tuple(t.shape)))
    return t.contiguous()


def same_device(*tensors):
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise RuntimeError("all tensors must be on the same device (%s vs %s)" % (dev, t.device))
    return dev
