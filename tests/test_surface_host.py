"""CPU: the host side of the surface step -- geom_surface_scan_f32, geom_surface_prepare_f32, geom_surface_finalize_w_f32,
geom_surface_gather_w_f32 (and their un-weighted wrappers) and the five tri entry points -- refuses bad arguments before
anything is enqueued, with the code it has always answered: -1 = GEOM_EINVAL, -2 = GEOM_ETOOBIG, -3 = GEOM_EUNSUPPORTED, 0 =
the empty-shape return.

Every row is one call with the named arguments changed.  The expected codes were recorded from the library as it stood before
the fused-launch rule, the workspace and scratch layouts and the tri entry points' checks were each gathered into one function
(csrc/tri_distance.hip, csrc/surface_layout.h) and are literals: where a call has several faults the FIRST failing check
decides, so the rows with two faults pin the order of the checks.  No row is a valid call: the pointers lie in a host buffer
that is never dereferenced, and a call that passed every check would be launched.  No answer depends on the device's LDS
size (nf + points per mesh stay below 10 000 or above 100 000).

A pointer value is written "pN" (slot N of the buffer, 128-byte aligned) or "pN+B" (B bytes further: misaligned).

The three size functions (geom_tri_distance_workspace_bytes, geom_surface_tail_counters_offset, geom_surface_order_words)
are pinned over a grid of shapes the same way: triangle counts that are no multiple of 64, query counts whose merged-keys
region is too small for the finalize tail's counters (offset 0)."""
import ctypes

import pytest

from geometrics_amd import _lib

_BUF = ctypes.create_string_buffer(32 * 128 + 128)
_BASE = (ctypes.addressof(_BUF) + 127) & ~127
WS_BYTES = 2854784          # geom_tri_distance_workspace_bytes(8, 3000, 5120)
TRUNC, FIX6, BRUTE, FMA, READY = (_lib.FLAG_REF_TAIL_TRUNC, _lib.FLAG_FIX_REGION6, _lib.FLAG_TRI_BRUTE_FORCE, _lib.FLAG_NN_FMA,
                                  _lib.FLAG_TRI_WS_READY)


def _value(v):
    if not isinstance(v, str):
        return v
    slot, _, off = v[1:].partition("+")
    return _BASE + 128 * int(slot) + int(off or 0)


def _args(base, edits):
    assert set(edits) <= set(base), set(edits) - set(base)
    return [_value(v) for v in dict(base, **edits).values()]


def _ids(v):
    return ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None


def _is_refusal(code, edits, empties):
    """Nothing here may reach a launch: a refusal, or the empty-shape return of an empty shape."""
    return code in (-1, -2, -3) or (code == 0 and any(edits.get(k) == 0 for k in empties))


# ---- geom_surface_scan_f32: eight meshes of 2562 vertices / 5120 faces, 3000 points each way, an order -- the fused branch,
# refused there for its NULL workspace.  cull = (gt_index, sample_index), tail = (choices, loss, want_order) -----------------
SCAN = dict(b=8, n_gt=3000, gt="p0", num=3000, points="p1", sq_gt="p2", idx_p="p3", sq_pred="p4", idx_g="p5", nv=2562, verts="p6",
            nf=5120, faces="p7", tri_order="p8", tri_dist="p9", option="p10", index="p11", sq="p12", closest="p13", weights="p14",
            u="p15", v="p16", coef_sample=1.0, coef_other=1.0, order_scratch="p17", flags=0, workspace=None, workspace_bytes=0)
_WS = dict(workspace="p20", workspace_bytes=WS_BYTES)      # passes the workspace check: only together with a later fault


def _scan_code(edits):
    edits = dict(edits)
    cull, tail = edits.pop("cull", None), edits.pop("tail", None)
    wrote = ctypes.c_int(7)
    c = _lib.SurfaceCull(None, _value(cull[0]), _value(cull[1]), None) if cull else None
    t = _lib.SurfaceTail(_value(tail[0]), 1.0, 1.0, tail[2], _value(tail[1]), 7) if tail else None
    code = _lib.lib().geom_surface_scan_f32(*_args(SCAN, edits), ctypes.byref(wrote), ctypes.byref(c) if c else None,
                                            ctypes.byref(t) if t else None, None)
    assert wrote.value == 0 and (t is None or t.finalized == 0)        # both out-values are cleared before the first check
    return code


# ---- geom_surface_prepare_f32: the same shape -- fused, refused for its 16-byte workspace.  cull = sample_index -------------
PREPARE = dict(b=8, nv=2562, verts="p0", nf=5120, faces="p1", num=3000, rng_state="p2", choices="p3", u="p4", v="p5", points="p6",
               n_gt=3000, tri_order="p7", flags=0, workspace="p8", workspace_bytes=16)


def _prepare_code(edits):
    edits = dict(edits)
    cull = edits.pop("cull", None)
    prepared = ctypes.c_int(7)
    c = _lib.SurfaceCull(None, None, _value(cull), None) if cull else None
    code = _lib.lib().geom_surface_prepare_f32(*_args(PREPARE, edits), ctypes.byref(prepared), ctypes.byref(c) if c else None, None)
    assert prepared.value == 0
    return code


# ---- the finalize pass and the gather (a valid call each: every row carries a fault) ------------------------------------------
FINALIZE = dict(b=8, nf=5120, num=3000, choices="p0", u="p1", v="p2", points="p3", n_gt=3000, gt="p4", idx_g="p5", idx_p=None,
                index="p6", closest="p7", weights="p8", sq_sample="p9", sq_other="p10", scale_sample=1.0, scale_other=1.0,
                coef_sample=1.0, coef_other=1.0, want_order=1, records_ready=0, order="p11", loss="p12")
GATHER = dict(b=8, nv=2562, nf=5120, vf_ptr="p0", vf_item="p1", num=3000, n_gt=3000, has_other=1, order="p2", grad="p3",
              grad_verts="p4")


def _finalize_codes(edits):
    a = _args(FINALIZE, edits)
    return _lib.lib().geom_surface_finalize_w_f32(*a, None, None), _lib.lib().geom_surface_finalize_f32(*a, None)


def _gather_codes(edits):
    a = _args(GATHER, edits)
    return _lib.lib().geom_surface_gather_w_f32(*a[:-1], None, a[-1], None), _lib.lib().geom_surface_gather_f32(*a, None)


# ---- the tri entry points: corner arrays (soup) or vertices + faces (indexed); the _WS bases are valid but for their workspace ---
SOUP = dict(b=8, n=3000, xyz="p0", m=5120, tri1="p1", tri2="p2", tri3="p3", order=None, dist="p4", point="p5", index="p6", flags=0,
            workspace=None, workspace_bytes=0)
INDEXED = dict(b=8, n=3000, xyz="p0", nv=2562, verts="p1", nf=5120, faces="p2", order=None, dist="p4", point="p5", index="p6",
               sqdist="p9", closest="p10", weights="p11", flags=0, workspace=None, workspace_bytes=0)


def _without(args, *names):
    return [_value(v) for k, v in args.items() if k not in names]


def _soup_codes(edits, plain=True):
    a = dict(SOUP, **edits)
    assert set(a) == set(SOUP)
    ws = _lib.lib().geom_tri_distance_ws_f32(*_without(a), None)
    return (_lib.lib().geom_tri_distance_f32(*_without(a, "order", "workspace", "workspace_bytes"), None), ws) if plain else ws


def _soup_ws_code(edits):
    return _soup_codes(edits, plain=False)


def _indexed_codes(edits, plain=True):
    a = dict(INDEXED, **edits)
    assert set(a) == set(INDEXED)
    L = _lib.lib()
    ws = (L.geom_tri_distance_indexed_ws_f32(*_without(a, "sqdist", "closest", "weights"), None), L.geom_tri_surface_fwd_f32(*_without(a), None))
    return ((L.geom_tri_distance_indexed_f32(*_without(a, "order", "sqdist", "closest", "weights", "workspace", "workspace_bytes"), None),) + ws
            if plain else ws)


def _indexed_ws_codes(edits):
    return _indexed_codes(edits, plain=False)


def _surface_fwd_code(edits):
    return _indexed_codes(edits, plain=False)[1]


# (edits on top of SCAN, code)
SCAN_ROWS = [
    ({}, -1),
    ({'b': -1}, -1),
    ({'n_gt': -1}, -1),
    ({'num': -1}, -1),
    ({'nf': -1}, -1),
    ({'nv': -1}, -1),
    ({'b': 0}, 0),
    ({'b': 0, 'gt': None}, 0),
    ({'b': 0, 'n_gt': -1}, -1),
    ({'n_gt': 0}, -1),
    ({'num': 0}, -1),
    ({'gt': None}, -1),
    ({'points': None}, -1),
    ({'sq_gt': None}, -1),
    ({'idx_p': None}, -1),
    ({'sq_pred': None}, -1),
    ({'idx_g': None}, -1),
    ({'faces': None}, -1),
    ({'tri_dist': None}, -1),
    ({'option': None}, -1),
    ({'index': None}, -1),
    ({'sq': None}, -1),
    ({'closest': None}, -1),
    ({'weights': None}, -1),
    ({'nf': 0}, -1),
    ({'nv': 0}, -1),
    ({'u': None}, -1),
    ({'v': None}, -1),
    ({'order_scratch': 'p17+4'}, -1),
    ({'order_scratch': None}, -1),
    ({'order_scratch': None, 'u': None, 'v': None}, -1),
    ({'b': 65536}, -2),
    ({'nf': 67108864}, -2),
    ({'b': 65536, 'gt': None}, -1),
    ({'b': 65536, 'u': None}, -1),
    ({'nf': 67108864, 'weights': None}, -1),
    ({'flags': 9}, -1),
    ({'flags': 9, 'b': 65536}, -2),
    ({'b': 65535, 'num': 600000}, -2),
    ({'b': 65535, 'num': 600000, 'flags': 9}, -1),
    ({'b': 65535, 'num': 600000, 'u': None}, -1),
    ({'workspace': 'p20', 'workspace_bytes': 16}, -1),
    ({'workspace': 'p20', 'workspace_bytes': 2854783}, -1),
    ({'workspace': 'p20+4', 'workspace_bytes': 2854784}, -1),
    ({'flags': 2}, -1),
    ({'flags': 8}, -1),
    ({'flags': 16}, -1),
    ({'n_gt': 2048}, -1),
    ({'verts': None, 'nf': -1}, -1),
    ({'workspace': 'p20', 'workspace_bytes': 2854784, 'flags': 16, 'cull': ('p21+4', 'p22')}, -1),
    ({'workspace': 'p20', 'workspace_bytes': 2854784, 'flags': 16, 'cull': ('p21', 'p22+8')}, -1),
    ({'workspace': 'p20', 'workspace_bytes': 2854784, 'flags': 16, 'tail': ('p23', None, 0)}, -1),
    ({'workspace': 'p20', 'workspace_bytes': 2854784, 'flags': 16, 'tail': (None, 'p24', 0)}, -1),
    ({'workspace': 'p20', 'workspace_bytes': 2854784, 'flags': 16, 'tail': ('p23', 'p24', 1), 'order_scratch': None}, -1),
    ({'workspace': 'p20', 'workspace_bytes': 2854784, 'flags': 16, 'cull': ('p21+4', 'p22'), 'tail': ('p23', None, 0)}, -1),
    ({'tri_order': None}, -1),
    ({'flags': 1}, -1),
    ({'n_gt': 1984}, -1),
    ({'b': 1}, -1),
    ({'b': 1, 'workspace': 'p20', 'workspace_bytes': 16}, -1),
    ({'tri_order': None, 'workspace': 'p20+4', 'workspace_bytes': 2854784}, -1),
]

# (edits on top of PREPARE, code)
PREPARE_ROWS = [
    ({}, -1),
    ({'b': -1}, -1),
    ({'nv': -1}, -1),
    ({'nf': -1}, -1),
    ({'num': -1}, -1),
    ({'n_gt': -1}, -1),
    ({'nf': 16385}, -3),
    ({'nf': 16385, 'b': -1}, -1),
    ({'nf': 16385, 'b': 0}, -3),
    ({'nf': 16385, 'verts': None}, -3),
    ({'b': 0}, 0),
    ({'num': 0}, 0),
    ({'num': 0, 'verts': None}, 0),
    ({'b': 0, 'workspace': None}, 0),
    ({'nf': 0}, -1),
    ({'verts': None}, -1),
    ({'faces': None}, -1),
    ({'rng_state': None}, -1),
    ({'choices': None}, -1),
    ({'u': None}, -1),
    ({'v': None}, -1),
    ({'b': 65536}, -2),
    ({'b': 65536, 'verts': None}, -1),
    ({'b': 65536, 'nf': 16385}, -3),
    ({'workspace_bytes': 2854783}, -1),
    ({'workspace': 'p8+4', 'workspace_bytes': 2854784}, -1),
    ({'flags': 2}, -1),
    ({'flags': 8}, -1),
    ({'flags': 16}, -1),
    ({'n_gt': 2048}, -1),
    ({'points': None}, -1),
    ({'workspace_bytes': 2854784, 'cull': 'p9+4'}, -1),
    ({'workspace_bytes': 2854784, 'cull': 'p9+8', 'flags': 2}, -1),
    ({'workspace_bytes': 16, 'cull': 'p9+4'}, -1),
]

# (edits on top of FINALIZE, code of geom_surface_finalize_w_f32, code of geom_surface_finalize_f32)
FINALIZE_ROWS = [
    ({'b': -1}, -1, -1),
    ({'nf': -1}, -1, -1),
    ({'num': -1}, -1, -1),
    ({'n_gt': -1}, -1, -1),
    ({'loss': None}, -1, -1),
    ({'order': None}, -1, -1),
    ({'order': 'p11+4'}, -1, -1),
    ({'b': 0}, 0, 0),
    ({'b': 0, 'loss': None}, -1, -1),
    ({'b': 0, 'sq_sample': None}, 0, 0),
    ({'b': -1, 'loss': None}, -1, -1),
    ({'sq_sample': None}, -1, -1),
    ({'sq_other': None}, -1, -1),
    ({'idx_p': 'p13'}, -1, -1),
    ({'b': 65536}, -2, -2),
    ({'b': 65536, 'idx_p': 'p13'}, -1, -1),
    ({'b': 65536, 'sq_other': None}, -1, -1),
    ({'num': 1073741824, 'n_gt': 1073741824}, -2, -2),
    ({'num': 1073741824, 'n_gt': 1073741824, 'b': 65536}, -2, -2),
    ({'num': 1073741824, 'n_gt': 1073741824, 'choices': None}, -2, -2),
    ({'choices': None}, -1, -1),
    ({'u': None}, -1, -1),
    ({'v': None}, -1, -1),
    ({'points': None}, -1, -1),
    ({'gt': None}, -1, -1),
    ({'idx_g': None}, -1, -1),
    ({'closest': None}, -1, -1),
    ({'weights': None}, -1, -1),
    ({'nf': 100000}, -3, -3),
    ({'nf': 100000, 'choices': None}, -1, -1),
    ({'nf': 100000, 'weights': None}, -1, -1),
    ({'num': 100000}, -3, -3),
    ({'sq_sample': None, 'idx_p': 'p13'}, -1, -1),
]

# (edits on top of GATHER, code of geom_surface_gather_w_f32, code of geom_surface_gather_f32)
GATHER_ROWS = [
    ({'b': -1}, -1, -1),
    ({'nv': -1}, -1, -1),
    ({'nf': -1}, -1, -1),
    ({'num': -1}, -1, -1),
    ({'n_gt': -1}, -1, -1),
    ({'b': 0}, 0, 0),
    ({'nv': 0}, 0, 0),
    ({'nv': 0, 'order': None}, 0, 0),
    ({'b': 0, 'vf_ptr': None}, 0, 0),
    ({'b': -1, 'nv': 0}, -1, -1),
    ({'vf_ptr': None}, -1, -1),
    ({'vf_item': None}, -1, -1),
    ({'order': None}, -1, -1),
    ({'grad_verts': None}, -1, -1),
    ({'order': 'p2+4'}, -1, -1),
    ({'b': 65536}, -2, -2),
    ({'b': 65536, 'order': None}, -1, -1),
    ({'b': 65536, 'order': 'p2+8'}, -1, -1),
]

# (edits on top of SOUP, code of geom_tri_distance_f32, code of geom_tri_distance_ws_f32)
SOUP_ROWS = [
    ({'b': -1}, -1, -1),
    ({'n': -1}, -1, -1),
    ({'m': -1}, -1, -1),
    ({'b': 0}, 0, 0),
    ({'n': 0}, 0, 0),
    ({'n': 0, 'm': 0}, 0, 0),
    ({'b': 0, 'm': -1}, -1, -1),
    ({'b': 0, 'xyz': None}, 0, 0),
    ({'m': 0}, -1, -1),
    ({'xyz': None}, -1, -1),
    ({'tri1': None}, -1, -1),
    ({'tri2': None}, -1, -1),
    ({'tri3': None}, -1, -1),
    ({'dist': None}, -1, -1),
    ({'point': None}, -1, -1),
    ({'index': None}, -1, -1),
    ({'b': 65536}, -2, -2),
    ({'m': 67108864}, -2, -2),
    ({'b': 65536, 'xyz': None}, -1, -1),
    ({'m': 67108864, 'index': None}, -1, -1),
    ({'m': 0, 'b': 65536}, -1, -1),
    ({'flags': 4, 'dist': None}, -1, -1),
    ({'flags': 4, 'b': 65536}, -2, -2),
]

# (edits on top of SOUP_WS: a valid call but for its workspace, code of geom_tri_distance_ws_f32)
SOUP_WS_ROWS = [
    ({}, -1),
    ({'order': 'p7'}, -1),
    ({'workspace': 'p20', 'workspace_bytes': 16}, -1),
    ({'workspace': 'p20+4', 'workspace_bytes': 2854784}, -1),
    ({'order': 'p7', 'workspace': 'p20', 'workspace_bytes': 2854783}, -1),
    ({'flags': 3}, -1),
    ({'n': 100}, -1),
]

# (edits on top of INDEXED, codes of geom_tri_distance_indexed_f32, geom_tri_distance_indexed_ws_f32, geom_tri_surface_fwd_f32)
INDEXED_ROWS = [
    ({'b': -1}, -1, -1, -1),
    ({'n': -1}, -1, -1, -1),
    ({'nf': -1}, -1, -1, -1),
    ({'nv': -1}, -1, -1, -1),
    ({'b': 0}, 0, 0, 0),
    ({'n': 0}, 0, 0, 0),
    ({'n': 0, 'nf': 0}, 0, 0, 0),
    ({'b': 0, 'nv': -1}, -1, -1, -1),
    ({'b': 0, 'verts': None}, 0, 0, 0),
    ({'nf': 0}, -1, -1, -1),
    ({'nv': 0}, -1, -1, -1),
    ({'xyz': None}, -1, -1, -1),
    ({'verts': None}, -1, -1, -1),
    ({'faces': None}, -1, -1, -1),
    ({'dist': None}, -1, -1, -1),
    ({'point': None}, -1, -1, -1),
    ({'index': None}, -1, -1, -1),
    ({'b': 65536}, -2, -2, -2),
    ({'nf': 67108864}, -2, -2, -2),
    ({'b': 65536, 'faces': None}, -1, -1, -1),
    ({'nf': 67108864, 'point': None}, -1, -1, -1),
    ({'nv': 0, 'b': 65536}, -1, -1, -1),
    ({'flags': 4, 'verts': None}, -1, -1, -1),
    ({'flags': 4, 'nf': 67108864}, -2, -2, -2),
]

# (edits on top of INDEXED_WS, codes of geom_tri_distance_indexed_ws_f32, geom_tri_surface_fwd_f32)
INDEXED_WS_ROWS = [
    ({}, -1, -1),
    ({'order': 'p7'}, -1, -1),
    ({'workspace': 'p20', 'workspace_bytes': 16}, -1, -1),
    ({'workspace': 'p20+4', 'workspace_bytes': 2854784}, -1, -1),
    ({'order': 'p7', 'workspace': 'p20', 'workspace_bytes': 2854783}, -1, -1),
    ({'flags': 3}, -1, -1),
    ({'n': 100}, -1, -1),
]

# what only geom_tri_surface_fwd_f32 checks: (edits on top of INDEXED_WS, code)
SURFACE_FWD_ROWS = [
    ({'sqdist': None}, -1),
    ({'closest': None}, -1),
    ({'weights': None}, -1),
    ({'sqdist': None, 'b': 65536}, -1),
    ({'weights': None, 'nf': 67108864}, -1),
    ({'sqdist': None, 'b': 0}, 0),
    ({'sqdist': None, 'nf': 0}, -1),
]

# sizes: rows b = (1, 3, 8), columns (n, m) for n in (0, 47, 48, 3000) for m in (1, 64, 65, 5120, 5121)
SIZE_B, SIZE_N, SIZE_M = (1, 3, 8), (0, 47, 48, 3000), (1, 64, 65, 5120, 5121)
WORKSPACE_BYTES = [[4208, 4208, 8368, 332848, 337008, 4584, 4584, 8744, 333224, 337384, 4592, 4592, 8752, 333232, 337392, 28208, 28208, 32368, 356848, 361008],
 [12624, 12624, 25104, 998544, 1011024, 13752, 13752, 26232, 999672, 1012152, 13776, 13776, 26256, 999696, 1012176, 84624, 84624, 97104, 1070544,
  1083024],
 [33664, 33664, 66944, 2662784, 2696064, 36672, 36672, 69952, 2665792, 2699072, 36736, 36736, 70016, 2665856, 2699136, 225664, 225664, 258944,
  2854784, 2888064]]
TAIL_COUNTERS_OFFSET = [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4208, 4208, 8368, 332848, 337008, 4208, 4208, 8368, 332848, 337008],
 [0, 0, 0, 0, 0, 12624, 12624, 25104, 998544, 1011024, 12624, 12624, 25104, 998544, 1011024, 12624, 12624, 25104, 998544, 1011024],
 [0, 0, 0, 0, 0, 33664, 33664, 66944, 2662784, 2696064, 33664, 33664, 66944, 2662784, 2696064, 33664, 33664, 66944, 2662784, 2696064]]
ORDER_NF, ORDER_POINTS = (0, 320, 5120), ((0, 0), (1, 5), (2048, 1985), (3000, 3000))
ORDER_WORDS = [[8, 72, 44368, 66008, 328, 392, 44688, 66328, 5128, 5192, 49488, 71128],
 [8, 208, 133096, 198008, 968, 1168, 134056, 198968, 15368, 15568, 148456, 213368],
 [20, 548, 354924, 528020, 2580, 3108, 357484, 530580, 40980, 41508, 395884, 568980]]


@pytest.mark.parametrize("edits,code", SCAN_ROWS, ids=_ids)
def test_scan_refusals(edits, code):
    assert _is_refusal(code, edits, ("b",))
    assert _scan_code(edits) == code


@pytest.mark.parametrize("edits,code", PREPARE_ROWS, ids=_ids)
def test_prepare_refusals(edits, code):
    assert _is_refusal(code, edits, ("b", "num"))
    assert _prepare_code(edits) == code


@pytest.mark.parametrize("edits,weighted,plain", FINALIZE_ROWS, ids=_ids)
def test_finalize_refusals(edits, weighted, plain):
    assert edits and _is_refusal(weighted, edits, ("b",)) and plain == weighted
    assert _finalize_codes(edits) == (weighted, plain)


@pytest.mark.parametrize("edits,weighted,plain", GATHER_ROWS, ids=_ids)
def test_gather_refusals(edits, weighted, plain):
    assert edits and _is_refusal(weighted, edits, ("b", "nv")) and plain == weighted
    assert _gather_codes(edits) == (weighted, plain)


@pytest.mark.parametrize("edits,plain,ws", SOUP_ROWS, ids=_ids)
def test_soup_refusals(edits, plain, ws):
    assert edits and _is_refusal(plain, edits, ("b", "n")) and _is_refusal(ws, edits, ("b", "n"))
    assert _soup_codes(edits) == (plain, ws)


@pytest.mark.parametrize("edits,plain,ws,surface", INDEXED_ROWS, ids=_ids)
def test_indexed_refusals(edits, plain, ws, surface):
    assert edits and all(_is_refusal(c, edits, ("b", "n")) for c in (plain, ws, surface))
    assert _indexed_codes(edits) == (plain, ws, surface)


@pytest.mark.parametrize("edits,code", SOUP_WS_ROWS, ids=_ids)
def test_soup_workspace_refusals(edits, code):
    assert code == -1 and not edits.get("flags", 0) & BRUTE        # (the brute-force scan takes no workspace: it would launch)
    assert _soup_ws_code(edits) == code


@pytest.mark.parametrize("edits,ws,surface", INDEXED_WS_ROWS, ids=_ids)
def test_indexed_workspace_refusals(edits, ws, surface):
    assert ws == -1 and surface == -1 and not edits.get("flags", 0) & BRUTE
    assert _indexed_ws_codes(edits) == (ws, surface)


@pytest.mark.parametrize("edits,code", SURFACE_FWD_ROWS, ids=_ids)
def test_surface_fwd_refusals(edits, code):
    assert _is_refusal(code, edits, ("b", "n"))
    assert _surface_fwd_code(edits) == code


def test_workspace_and_scratch_sizes():
    L = _lib.lib()
    assert L.geom_tri_distance_workspace_bytes(8, 3000, 5120) == 2854784
    assert L.geom_surface_tail_counters_offset(8, 3000, 5120) == 2662784
    assert L.geom_surface_order_words(8, 5120, 3000, 3000) == 568980
    for i, b in enumerate(SIZE_B):
        shapes = [(n, m) for n in SIZE_N for m in SIZE_M]
        assert [L.geom_tri_distance_workspace_bytes(b, n, m) for n, m in shapes] == WORKSPACE_BYTES[i]
        assert [L.geom_surface_tail_counters_offset(b, n, m) for n, m in shapes] == TAIL_COUNTERS_OFFSET[i]
        assert [L.geom_surface_order_words(b, nf, num, n_gt) for nf in ORDER_NF for num, n_gt in ORDER_POINTS] == ORDER_WORDS[i]
    # the counters sit behind the records, inside the workspace, wherever they fit; nothing is sized for an empty or negative shape
    assert any(0 in row for row in TAIL_COUNTERS_OFFSET) and any(max(row) > 0 for row in TAIL_COUNTERS_OFFSET)
    for b, n, m in ((0, 3000, 5120), (-1, 3000, 5120), (8, 3000, 0), (8, 3000, -1), (8, -1, 5120)):
        assert L.geom_tri_distance_workspace_bytes(b, n, m) == 0 and L.geom_surface_tail_counters_offset(b, n, m) == 0
    assert L.geom_surface_tail_counters_offset(8, 0, 5120) == 0
    for b, nf, num, n_gt in ((0, 5120, 3000, 3000), (-1, 5120, 3000, 3000), (8, -1, 3000, 3000), (8, 5120, -1, 3000), (8, 5120, 3000, -1)):
        assert L.geom_surface_order_words(b, nf, num, n_gt) == 0
