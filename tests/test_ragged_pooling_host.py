"""CPU: the grouping of a union's vertices (ragged.group_vertices, torch ops) against numpy, that group_faces still returns what
it did, the three ragged pooling entry points as the header declares them, their workspace size against the documented layout,
the limits they look at before any pointer, and utils.ragged_pooling's argument checks."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from geometrics_amd import _header, _lib, ragged, utils
from ragged_loss_helpers import batch_a, batch_b

NAMES = ("geom_pool_features_ragged_fwd_f32", "geom_pool_features_ragged_bwd_workspace_bytes", "geom_pool_features_ragged_bwd_f32")
EINVAL, ETOOBIG, EUNSUPPORTED = (_header.CONSTANTS[k] for k in ("EINVAL", "ETOOBIG", "EUNSUPPORTED"))


def interleaved_ids(b=4, n=300, seed=5):
    """n ids of b meshes in no order, mesh 2 empty, and a handful outside [0, b) on both sides."""
    rng = np.random.default_rng(seed)
    ids = rng.choice([0, 1, 3], size=n).astype(np.int64)
    ids[rng.choice(n, 9, replace=False)] = [-1, -7, b, b + 3, -2, 2 ** 40, b, -1, -(2 ** 35)]
    return ids


def numpy_grouping(ids, b):
    clamped = np.clip(ids, -1, b)
    order = np.argsort(clamped, kind="stable")
    return order, np.searchsorted(clamped[order], np.arange(b + 1), side="left")


@pytest.mark.parametrize("dtype", (torch.int64, torch.int32))
def test_group_vertices_equals_its_numpy_restatement(dtype):
    b = 4
    ids = interleaved_ids(b)
    if dtype == torch.int32:
        ids = np.clip(ids, -2 ** 31, 2 ** 31 - 1)
    want_list, want_off = numpy_grouping(ids, b)
    assert not (np.diff(ids) >= 0).all()
    t = torch.from_numpy(ids).to(dtype)
    vert_list, vert_off = ragged.group_vertices(t, b)
    assert vert_list.dtype == vert_off.dtype == torch.int32 and vert_list.is_contiguous() and vert_off.is_contiguous()
    np.testing.assert_array_equal(vert_list.numpy(), want_list)
    np.testing.assert_array_equal(vert_off.numpy(), want_off)
    lo, hi = int(vert_off[0]), int(vert_off[b])
    assert lo == (ids < 0).sum() and len(ids) - hi == (ids >= b).sum()           # the vertices of no mesh stand outside [lo, hi)
    assert int(vert_off[3]) == int(vert_off[2])                                     # mesh 2 is empty
    for m in range(b):                                                             # a mesh's vertices, ascending
        span = vert_list[int(vert_off[m]):int(vert_off[m + 1])].numpy()
        np.testing.assert_array_equal(span, np.flatnonzero(ids == m))


def test_group_vertices_is_cached_per_tensor_object_and_version():
    t = torch.from_numpy(interleaved_ids())
    first = ragged.group_vertices(t, 4)
    assert ragged.group_vertices(t, 4)[0] is first[0] and ragged.group_vertices(t, 4)[1] is first[1]
    assert ragged.group_vertices(t.clone(), 4)[0] is not first[0]
    assert ragged.group_vertices(t, 6)[0] is not first[0]                           # another mesh count is another entry
    np.testing.assert_array_equal(ragged.group_vertices(t, 6)[1].numpy()[:4], first[1].numpy()[:4])
    t[0] = 1 - t[0].clamp(0, 1)                                                     # an in-place change drops the entry
    again = ragged.group_vertices(t, 4)
    assert again[0] is not first[0]
    np.testing.assert_array_equal(again[0].numpy(), numpy_grouping(t.numpy(), 4)[0])
    with pytest.raises(RuntimeError, match="one-dimensional int32 or int64"):
        ragged.group_vertices(t.float(), 4)
    with pytest.raises(RuntimeError, match="one-dimensional int32 or int64"):
        ragged.group_vertices(t.view(-1, 2), 4)


@pytest.mark.parametrize("make", [batch_a, batch_b])
def test_group_faces_returns_what_it_did(make):
    """The fixtures of test_ragged_loss_host.py: the list and the offsets, with and without the faces as a key, and the
    UNCLAMPED order of ids outside the batch (group_faces sorts the ids as they are)."""
    rb = make()
    want_list, want_off = rb.grouping()
    faces, ids = torch.from_numpy(rb.faces), torch.from_numpy(rb.face_mesh)
    for got in (ragged.group_faces(ids, rb.b, faces), ragged.group_faces(ids, rb.b)):
        assert got[0].dtype == got[1].dtype == torch.int32
        np.testing.assert_array_equal(got[0].numpy(), want_list)
        np.testing.assert_array_equal(got[1].numpy(), want_off)
    stray = torch.tensor([1, -2, 0, 7, -5, 1, 9, 0], dtype=torch.int64)
    face_list, face_off = ragged.group_faces(stray, 2)
    np.testing.assert_array_equal(face_list.numpy(), [4, 1, 2, 7, 0, 5, 3, 6])
    np.testing.assert_array_equal(face_off.numpy(), [2, 4, 6])


def test_the_ragged_pooling_symbols_are_declared_and_exported_and_the_abi_version_stands():
    L = _lib.lib()
    assert L.geom_abi_version() == 16 == _lib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout
    exported = {line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in "Tt"}
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in exported, name
    I, P, L64, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
    same = lambda got, want: len(got) == len(want) and all(ctypes.sizeof(g) == ctypes.sizeof(w) and (g is P) == (w is P)
                                                           for g, w in zip(got, want))
    restype, argtypes = _header.PROTOTYPES[NAMES[0]]
    assert restype is I and same(argtypes, [I, I, P, P, P, P, P, I, P, P, P, P, L64, P])
    assert [p for p, _, _ in _header.PARAMETERS[NAMES[0]]] == ["b", "vt", "verts", "vert_mesh", "vert_list", "cam_mat", "cam_pos", "levels",
                                                              "blocks", "channels", "dims", "out", "out_ld", "stream"]
    restype, argtypes = _header.PROTOTYPES[NAMES[1]]
    assert ctypes.sizeof(restype) == ctypes.sizeof(Z) and same(argtypes, [I, I, I, P])
    restype, argtypes = _header.PROTOTYPES[NAMES[2]]
    assert restype is I and same(argtypes, [I, I, P, P, P, P, P, P, I, P, P, P, P, L64, P, P, P, Z, P])
    assert [p for p, _, _ in _header.PARAMETERS[NAMES[2]]] == ["b", "vt", "verts", "vert_mesh", "vert_list", "vert_off", "cam_mat", "cam_pos",
                                                              "levels", "blocks", "channels", "dims", "grad_out", "grad_ld", "grad_blocks",
                                                              "grad_verts", "workspace", "workspace_bytes", "stream"]
    pointees = {p: (t, d) for p, t, d in _header.PARAMETERS[NAMES[2]]}
    assert pointees["vert_mesh"] == pointees["vert_list"] == pointees["vert_off"] == ("int", 1)
    assert pointees["verts"] == ("float", 1) and pointees["blocks"] == ("float", 2) and pointees["grad_blocks"] == ("float", 2)


@pytest.mark.parametrize("b, vt, dims", [(16, 7712, (56, 28, 14, 7)), (3, 101, (5, 9, 40, 1))])
def test_the_workspace_size_is_the_documented_layout(b, vt, dims):
    """geom_hip.h: the offsets of all meshes padded to 16 bytes; 4 * vt ids and 4 * vt weights per LEVEL, padded to 16 bytes
    together with them; the per-chunk sums [32][vt][2]."""
    pad = lambda n: (n + 15) // 16 * 16
    offsets = pad(b * sum(d * d + 1 for d in dims) * 4)
    lists = pad(offsets + len(dims) * 4 * vt * (4 + 4))
    want = lists + 32 * vt * 2 * 4
    got = _lib.lib().geom_pool_features_ragged_bwd_workspace_bytes(b, vt, len(dims), (ctypes.c_int * len(dims))(*dims))
    assert got == want
    batched = _lib.lib().geom_pool_features_bwd_workspace_bytes(1, vt, len(dims), (ctypes.c_int * len(dims))(*dims))
    assert got - batched == offsets - pad(sum(d * d + 1 for d in dims) * 4)      # one mesh's layout but for the other meshes' offsets
    assert _lib.lib().geom_pool_features_ragged_bwd_workspace_bytes(b, 0, len(dims), (ctypes.c_int * len(dims))(*dims)) == 0


def ragged_calls(b, vt, channels, dims, pointer):
    L = _lib.lib()
    n = len(dims)
    ch, dm = (ctypes.c_int * n)(*channels), (ctypes.c_int * n)(*dims)
    fwd = L.geom_pool_features_ragged_fwd_f32(b, vt, pointer, pointer, pointer, pointer, pointer, n, None, ch, dm, pointer, 0, None)
    bwd = L.geom_pool_features_ragged_bwd_f32(b, vt, pointer, pointer, pointer, pointer, pointer, pointer, n, None, ch, dm, pointer, 0,
                                              None, pointer, pointer, 0, None)
    return fwd, bwd


def test_the_limits_are_looked_at_before_any_pointer():
    """Null device pointers everywhere (and a null host array of map pointers): the size limits answer first."""
    assert ragged_calls(2, 100, (4, 4), (65, 7), None) == (EUNSUPPORTED, EUNSUPPORTED)            # maps up to 64 x 64
    assert ragged_calls(2, 100, (4, 4), (7, 128), None) == (EUNSUPPORTED, EUNSUPPORTED)
    # all meshes' planes of a map are one buffer with 32-bit offsets: 64 * 4096 * 64 * 64 * 4 = 2^32 is one byte too many
    assert ragged_calls(64, 100, (4096,), (64,), None) == (ETOOBIG, ETOOBIG)
    assert ragged_calls(64, 100, (8, 4096), (7, 64), None) == (ETOOBIG, ETOOBIG)
    assert ragged_calls(63, 100, (4096,), (64,), None) == (EINVAL, EINVAL)                        # inside the limit: the null pointers
    assert ragged_calls(-1, 100, (4,), (7,), None) == (EINVAL, EINVAL)
    assert ragged_calls(2, -1, (4,), (7,), None) == (EINVAL, EINVAL)
    assert ragged_calls(2, 100, (0,), (7,), None) == (EINVAL, EINVAL)
    assert ragged_calls(2, 100, (4,) * 9, (7,) * 9, None) == (EINVAL, EINVAL)                     # more than GEOM_POOL_MAX_LEVELS maps


def test_ragged_pooling_refuses_bad_arguments_before_any_launch(monkeypatch):
    def no_launch(name, *args):
        raise AssertionError("%s was called" % name)

    monkeypatch.setattr(_lib, "call", no_launch)
    monkeypatch.setattr(_lib, "status", no_launch)
    b, vt = 3, 20
    ok = dict(blocks=[torch.zeros(b, 4, 7, 7), torch.zeros(b, 2, 5, 5)], verts_union=torch.zeros(vt, 3),
              vert_mesh=torch.zeros(vt, dtype=torch.int64), img_info=torch.tensor([[35.0, 20.0, 1.2]] * b))
    call = lambda **kw: utils.ragged_pooling(**{**ok, **kw})
    with pytest.raises(RuntimeError, match="fp32 \\[B, C, dim, dim\\]"):
        call(blocks=[ok["blocks"][0], ok["blocks"][1].double()])
    with pytest.raises(RuntimeError, match="fp32 \\[Vt,3\\]"):
        call(verts_union=ok["verts_union"].double())
    with pytest.raises(RuntimeError, match="fp32 \\[Vt,3\\]"):
        call(verts_union=torch.zeros(1, vt, 3))
    with pytest.raises(RuntimeError, match="int32 or int64"):
        call(vert_mesh=ok["vert_mesh"].float())
    with pytest.raises(RuntimeError, match="int32 or int64"):
        call(vert_mesh=ok["vert_mesh"].to(torch.int16))
    with pytest.raises(RuntimeError, match="cameras must be fp32"):
        call(img_info=ok["img_info"].double())
    with pytest.raises(RuntimeError, match="holds %d ids, the union %d vertices" % (vt - 1, vt)):
        call(vert_mesh=ok["vert_mesh"][:-1])
    with pytest.raises(RuntimeError, match="holds 3 images, the cameras 2"):
        call(img_info=ok["img_info"][:2])
    with pytest.raises(RuntimeError, match="holds 2 images, the cameras 3"):
        call(blocks=[ok["blocks"][0], ok["blocks"][1][:2]])
    with pytest.raises(RuntimeError, match="square planes"):
        call(blocks=[torch.zeros(b, 4, 7, 6)])
    with pytest.raises(RuntimeError, match="at least one feature map"):
        call(blocks=[])
