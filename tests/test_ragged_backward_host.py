"""CPU: what the ordered backward of the ragged surface loss is built from on the host -- ragged.face_positions and
ragged.vertex_faces (torch ops) against numpy, the scratch's words function against the layout it documents, the new entry
points refusing bad arguments with the header's codes before any launch (refusal paths and empty calls only: nothing is
launched here), and the validation of utils.ragged_point_to_surface's `weight`."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from geometrics_amd import _header, _lib, ops, ragged, utils
from ragged_loss_helpers import batch_a, batch_b

P = 16       # any non-null 16-byte aligned address: validation never dereferences
EINVAL, ETOOBIG, EUNSUPPORTED = (_header.CONSTANTS[k] for k in ("EINVAL", "ETOOBIG", "EUNSUPPORTED"))
NAMES = ("geom_surface_finalize_ragged_f32", "geom_surface_gather_ragged_f32")


def _positions(face_mesh, b):
    """numpy restatement: the position of every face in the stable sort by mesh id, -1 for an id outside [0, b)."""
    order = np.argsort(face_mesh, kind="stable")
    pos = np.empty(len(face_mesh), np.int32)
    pos[order] = np.arange(len(face_mesh), dtype=np.int32)
    pos[(face_mesh < 0) | (face_mesh >= b)] = -1
    return pos


@pytest.mark.parametrize("make", [batch_a, batch_b])
def test_face_positions_invert_the_face_list(make):
    rb = make()
    faces, ids = torch.from_numpy(rb.faces), torch.from_numpy(rb.face_mesh)
    pos = ragged.face_positions(ids, rb.b, faces)
    assert pos.dtype == torch.int32 and pos.is_contiguous() and pos.shape == ids.shape
    np.testing.assert_array_equal(pos.numpy(), _positions(rb.face_mesh, rb.b))
    face_list, face_off = ragged.group_faces(ids, rb.b, faces)
    assert isinstance(ragged.group_faces(ids, rb.b, faces), tuple) and len(ragged.group_faces(ids, rb.b, faces)) == 2
    np.testing.assert_array_equal(face_list[pos.long()].numpy(), np.arange(len(rb.face_mesh)))
    for m in range(rb.b):              # the position inside the mesh counts the mesh's faces in ascending union id
        own = rb.faces_of(m)[0]
        np.testing.assert_array_equal(pos.numpy()[own] - int(face_off[m]), np.arange(len(own)))
    # what ops derives from the grouping alone when no table is handed in
    np.testing.assert_array_equal(ops._face_positions(face_list, face_off).numpy(), pos.numpy())
    # cached per tensor objects and versions, like group_faces
    assert ragged.face_positions(ids, rb.b, faces) is pos
    assert ragged.face_positions(ids.clone(), rb.b, faces) is not pos
    # ids outside [0, b): a smaller mesh count leaves the last mesh's faces without a mesh, negative ids likewise
    fewer = ragged.face_positions(ids, rb.b - 1, faces)
    np.testing.assert_array_equal(fewer.numpy(), _positions(rb.face_mesh, rb.b - 1))
    assert int((fewer == -1).sum()) == rb.sizes[-1]
    shifted = rb.face_mesh - 1
    got = ragged.face_positions(torch.from_numpy(shifted), rb.b)
    np.testing.assert_array_equal(got.numpy(), _positions(shifted, rb.b))
    fl, fo = ragged.group_faces(torch.from_numpy(shifted), rb.b)
    np.testing.assert_array_equal(ops._face_positions(fl, fo).numpy(), got.numpy())
    ids[0] = (ids[0] + 1) % rb.b                                   # an in-place change drops the entry
    assert ragged.face_positions(ids, rb.b, faces) is not pos


def _vertex_faces(faces, nv):
    flat = faces.reshape(-1)
    order = np.argsort(flat, kind="stable")
    item = (((order // 3) << 2) | (order % 3)).astype(np.int32)
    ptr = np.searchsorted(flat[order], np.arange(nv + 1), side="left").astype(np.int32)
    return ptr, item


@pytest.mark.parametrize("make", [batch_a, batch_b])
def test_vertex_faces_without_host_reads_is_the_static_table(make):
    rb = make()
    nv = rb.verts.shape[0]
    faces = torch.from_numpy(rb.faces)
    vf_ptr, vf_item = ragged.vertex_faces(faces, nv)
    assert vf_ptr.dtype == vf_item.dtype == torch.int32 and vf_ptr.is_contiguous() and vf_item.is_contiguous()
    want_ptr, want_item = _vertex_faces(rb.faces, nv)
    np.testing.assert_array_equal(vf_ptr.numpy(), want_ptr)
    np.testing.assert_array_equal(vf_item.numpy(), want_item)
    old_ptr, old_item = ops.vertex_faces(faces.clone(), nv)         # the table with the two host reads
    assert torch.equal(vf_ptr, old_ptr) and torch.equal(vf_item, old_item)
    for vtx in (0, nv // 2, nv - 1):                                # every entry names a corner that is this vertex, ascending
        items = vf_item[vf_ptr[vtx]:vf_ptr[vtx + 1]].numpy()
        assert (np.diff(items) > 0).all()
        assert all(rb.faces[i >> 2, i & 3] == vtx for i in items)
    assert ragged.vertex_faces(faces, nv)[0] is vf_ptr and ragged.vertex_faces(faces, nv + 1)[0] is not vf_ptr
    # a corner outside [0, nv): in front of vf_ptr[0] or behind vf_ptr[nv], never inside a row
    bad = rb.faces.copy()
    bad[3, 1], bad[5, 2] = -7, nv + 3
    ptr, item = ragged.vertex_faces(torch.from_numpy(bad), nv)
    want_ptr, want_item = _vertex_faces(bad, nv)
    np.testing.assert_array_equal(ptr.numpy(), want_ptr)
    np.testing.assert_array_equal(item.numpy(), want_item)
    assert int(ptr[0]) == 1 and int(ptr[nv]) == bad.size - 1
    walked = item[int(ptr[0]):int(ptr[nv])].numpy()
    assert ((3 << 2) | 1) not in walked and ((5 << 2) | 2) not in walked
    with pytest.raises(RuntimeError):
        ops.vertex_faces(torch.from_numpy(bad), nv)
    with pytest.raises(RuntimeError):
        ragged.vertex_faces(faces.to(torch.int32), nv)


def test_the_words_function_follows_the_layout():
    """pair[nft] int2 | fmesh[nft] | seg, pface, slot [b,cap] | pad to 4 | rec [b,cap,2] float4 | status [b+1, pad to 4]."""
    words = _lib.lib().geom_surface_order_ragged_words
    assert _header.PROTOTYPES["geom_surface_order_ragged_words"][0] is ctypes.c_int64
    for b, nft, num, n_gt in ((1, 1, 1, 1), (8, 3248, 1025, 130), (4, 1038, 8100, 130), (5, 1038, 1, 65), (16, 46000, 3000, 3000)):
        cap = num + n_gt
        ints = (3 * nft + 3 * b * cap + 3) // 4 * 4
        assert words(b, nft, num, n_gt) == ints + 8 * b * cap + (b + 1 + 3) // 4 * 4, (b, nft, num, n_gt)
        assert words(b, nft, num, n_gt) % 4 == 0
    assert words(3, 0, 2, 2) == 36 + 96 + 4                          # no faces: the per-point arrays alone
    for bad in ((0, 4, 1, 1), (-1, 4, 1, 1), (2, -1, 1, 1), (2, 4, -1, 1), (2, 4, 1, -1)):
        assert words(*bad) == 0


def test_the_face_cap_is_what_fits_beside_the_points():
    cap = _lib.lib().geom_surface_ragged_face_cap
    assert cap(-1, 1, 1) == EINVAL and cap(4, -1, 1) == EINVAL and cap(4, 1, -1) == EINVAL
    assert cap(100, 200, 60) == 100                                 # few faces: all of them
    fit = cap(1 << 30, 200, 60)                                     # what the ordering pass's LDS holds beside 260 points
    assert 0 < fit < (1 << 30) and cap(fit + 1, 200, 60) == fit and cap(fit, 200, 60) == fit
    assert cap(1 << 30, 201, 60) == fit - 1                          # a point costs what a face costs: one word
    assert cap(4, fit + 261, 0) == EUNSUPPORTED and cap(4, fit + 260, 0) == 0      # the points alone do not fit / just fit


def test_the_symbols_are_declared_and_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout
    exported = {line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in "Tt"}
    for name in NAMES + ("geom_surface_order_ragged_words", "geom_surface_ragged_face_cap"):
        assert name in _lib.declared_symbols() and name in exported, name
    for name in NAMES:
        restype, argtypes = _header.PROTOTYPES[name]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p        # a code back, the stream last
    assert [p for p, _, _ in _header.PARAMETERS[NAMES[0]]] == [
        "b", "nft", "face_list", "face_off", "face_pos", "num", "choices", "u", "v", "points", "n_gt", "gt", "idx_g", "idx_p", "index",
        "closest", "weights", "sq_sample", "sq_other", "scale_sample", "scale_other", "coef_sample", "coef_other", "order", "loss",
        "mesh_weight", "stream"]
    assert [p for p, _, _ in _header.PARAMETERS[NAMES[1]]] == ["b", "nv", "nft", "vf_ptr", "vf_item", "num", "n_gt", "order", "grad",
                                                              "mesh_weight", "grad_verts", "stream"]


def test_the_ragged_finalize_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(b=2, nft=4, face_list=P, face_off=P, face_pos=P, num=8, choices=P, u=P, v=P, points=P, n_gt=8, gt=P, idx_g=P, idx_p=None,
              index=P, closest=P, weights=P, sq_sample=P, sq_other=P, scale_sample=1.0, scale_other=1.0, coef_sample=1.0, coef_other=1.0,
              order=P, loss=P, mesh_weight=None)
    call = lambda **kw: L.geom_surface_finalize_ragged_f32(*{**ok, **kw}.values(), None)
    for size in ("b", "nft", "num", "n_gt"):
        assert call(**{size: -1}) == EINVAL, size
    for pointer in ("face_list", "face_off", "face_pos", "choices", "u", "v", "points", "gt", "idx_g", "closest", "weights", "sq_sample",
                    "sq_other", "order"):
        assert call(**{pointer: None}) == EINVAL, pointer
    assert call(order=P + 4) == EINVAL                               # misaligned scratch
    assert call(index=None) == EINVAL and call(idx_p=P) == EINVAL    # exactly one partner kind
    assert call(loss=None, mesh_weight=P) == EINVAL                  # the weighted loss has to go somewhere
    assert call(n_gt=0) == EINVAL                                    # samples without partners
    assert call(b=65536) == ETOOBIG and call(b=65535, num=1 << 14, n_gt=1 << 14) == ETOOBIG      # flat ids beyond 2^30
    assert call(num=1 << 20) == EUNSUPPORTED                         # the points alone do not fit the launch's LDS
    assert call(b=0) == 0
    assert call(b=0, face_list=None, face_off=None, face_pos=None, choices=None, u=None, v=None, points=None, gt=None, idx_g=None,
                index=None, closest=None, weights=None, sq_sample=None, sq_other=None, loss=None) == 0
    assert call(b=0, order=None) == EINVAL


def test_the_ragged_gather_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(b=2, nv=6, nft=4, vf_ptr=P, vf_item=P, num=8, n_gt=8, order=P, grad=None, mesh_weight=None, grad_verts=P)
    call = lambda **kw: L.geom_surface_gather_ragged_f32(*{**ok, **kw}.values(), None)
    for size in ("b", "nv", "nft", "num", "n_gt"):
        assert call(**{size: -1}) == EINVAL, size
    for pointer in ("vf_ptr", "vf_item", "order", "grad_verts"):
        assert call(**{pointer: None}) == EINVAL, pointer
    assert call(order=P + 8) == EINVAL
    assert call(b=65536) == ETOOBIG and call(b=65535, num=1 << 14, n_gt=1 << 14) == ETOOBIG
    assert call(b=0) == 0 and call(nv=0) == 0
    assert call(b=0, vf_ptr=None, vf_item=None, order=None, grad_verts=None) == 0


def test_weight_is_a_float_or_one_fp32_factor_per_mesh():
    """Refused on the host, in front of anything that needs a device."""
    rb = batch_b()
    verts, faces, ids = torch.from_numpy(rb.verts), torch.from_numpy(rb.faces), torch.from_numpy(rb.face_mesh)
    gt = torch.zeros(rb.b, 5, 3)
    for fn in (utils.ragged_point_to_surface, utils.ragged_point_to_point):
        for bad in (torch.ones(rb.b + 1), torch.ones(rb.b, 1), torch.ones(rb.b, dtype=torch.float64), torch.ones(rb.b, dtype=torch.int32),
                    "2", None, [1.0] * rb.b, True):
            with pytest.raises(RuntimeError, match="weight"):
                fn(verts, faces, ids, gt, num=4, weight=bad)
    assert ops.ragged_backward in ("ordered", "scatter")
