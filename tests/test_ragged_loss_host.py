"""CPU: the grouping of a ragged batch's faces (ragged.group_faces, torch ops) against numpy, and the two ragged entry points
of the surface loss -- declared, exported, refusing bad arguments with the header's codes before any launch (refusal paths and
empty calls only: nothing is launched here)."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from geometrics_amd import _header, _lib, ragged
from ragged_loss_helpers import batch_a, batch_b

P = 8        # any non-null address: validation never dereferences
NAMES = ("geom_draw_samples_ragged_f32", "geom_tri_distance_ragged_f32")
EINVAL = _header.CONSTANTS["EINVAL"]


@pytest.mark.parametrize("make", [batch_a, batch_b])
def test_group_faces_equals_its_numpy_restatement(make):
    rb = make()
    assert not (np.diff(rb.face_mesh) >= 0).all()                  # shuffled: the meshes interleave
    want_list, want_off = rb.grouping()
    faces, ids = torch.from_numpy(rb.faces), torch.from_numpy(rb.face_mesh)
    face_list, face_off = ragged.group_faces(ids, rb.b, faces)
    assert face_list.dtype == face_off.dtype == torch.int32 and face_list.is_contiguous() and face_off.is_contiguous()
    np.testing.assert_array_equal(face_list.numpy(), want_list)
    np.testing.assert_array_equal(face_off.numpy(), want_off)
    assert tuple(np.diff(want_off)) == rb.sizes
    for m in range(rb.b):                                          # inside a mesh positions ascend with the face id
        span = face_list[want_off[m]:want_off[m + 1]].numpy()
        np.testing.assert_array_equal(span, rb.faces_of(m)[0])
    # cached per tensor OBJECTS and versions; another mesh count is another entry; int32 ids group alike
    assert ragged.group_faces(ids, rb.b, faces)[0] is face_list
    assert ragged.group_faces(ids.clone(), rb.b, faces)[0] is not face_list
    np.testing.assert_array_equal(ragged.group_faces(ids, rb.b + 2, faces)[1].numpy(), np.concatenate((want_off, [want_off[-1]] * 2)))
    np.testing.assert_array_equal(ragged.group_faces(ids.to(torch.int32), rb.b)[0].numpy(), want_list)
    ids[0] = (ids[0] + 1) % rb.b                                   # an in-place change drops the entry
    assert ragged.group_faces(ids, rb.b, faces)[0] is not face_list


def test_face_mesh_follows_the_first_corner():
    rb = batch_b()
    vert_mesh = np.repeat(np.arange(rb.b), np.diff(rb.vert_off))
    got = ragged.face_mesh(torch.from_numpy(rb.faces), torch.from_numpy(vert_mesh))
    np.testing.assert_array_equal(got.numpy(), rb.face_mesh)


def test_the_ragged_symbols_are_declared_and_exported_and_the_abi_version_stands():
    L = _lib.lib()
    assert L.geom_abi_version() == 16 == _lib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout
    exported = {line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in "Tt"}
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in exported, name
        restype, argtypes = _header.PROTOTYPES[name]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p        # a code back, the stream last
    assert [p for p, _, _ in _header.PARAMETERS[NAMES[0]]] == ["b", "nv", "verts", "nf", "faces", "face_list", "face_off", "num", "uniforms",
                                                              "rng_state", "choices", "u", "v", "points", "stream"]
    assert [p for p, _, _ in _header.PARAMETERS[NAMES[1]]] == ["b", "n", "xyz", "nv", "verts", "nf", "faces", "face_list", "face_off", "dist",
                                                              "point", "index", "flags", "stream"]


def test_the_ragged_draw_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(b=2, nv=4, verts=P, nf=4, faces=P, face_list=P, face_off=P, num=8, uniforms=P, rng_state=None, choices=P, u=P, v=P, points=None)
    call = lambda **kw: L.geom_draw_samples_ragged_f32(*{**ok, **kw}.values(), None)
    for size in ("b", "nv", "nf", "num"):
        assert call(**{size: -1}) == EINVAL, size
    for pointer in ("verts", "faces", "face_list", "face_off", "choices", "u", "v"):
        assert call(**{pointer: None}) == EINVAL, pointer
    assert call(uniforms=P, rng_state=P) == EINVAL                  # exactly one source of uniforms
    assert call(uniforms=None, rng_state=None) == EINVAL
    assert call(nf=0) == EINVAL                                     # samples of a batch without faces
    assert call(b=0) == 0 and call(num=0) == 0                      # nothing to do
    assert call(b=0, verts=None, faces=None, face_list=None, face_off=None, uniforms=None, choices=None, u=None, v=None) == 0


def test_the_ragged_scan_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(b=2, n=8, xyz=P, nv=4, verts=P, nf=4, faces=P, face_list=P, face_off=P, dist=P, point=P, index=P, flags=0)
    call = lambda **kw: L.geom_tri_distance_ragged_f32(*{**ok, **kw}.values(), None)
    for size in ("b", "n", "nv", "nf"):
        assert call(**{size: -1}) == EINVAL, size
    for pointer in ("xyz", "verts", "faces", "face_list", "face_off", "dist", "point", "index"):
        assert call(**{pointer: None}) == EINVAL, pointer
    assert call(flags=_lib.FLAG_REF_TAIL_TRUNC) == EINVAL           # the truncation mode knows one shared face list
    assert call(flags=_lib.FLAG_REF_TAIL_TRUNC | _lib.FLAG_TRI_BRUTE_FORCE) == EINVAL
    assert call(nf=0) == EINVAL
    assert call(nf=1 << 26) == _header.CONSTANTS["ETOOBIG"]         # positions share the key's 28 bits with the region code
    assert call(b=0) == 0 and call(n=0) == 0                        # nothing to do
    assert call(n=0, xyz=None, verts=None, faces=None, face_list=None, face_off=None, dist=None, point=None, index=None) == 0
