"""CPU: the face-splitting entry points of csrc/face_split.hip are declared and exported, refuse bad arguments with the header's codes
before any launch (refusal paths only: nothing is launched here), the ABI version stands, and utils.split_info / calc_face_list
refuse what they document."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from geometrics_amd import _header, _lib, layers, meshgen, utils

P = 8        # any non-null address: validation never dereferences
NAMES = ("geom_face_curvature_f32", "geom_face_select_f32", "geom_face_split_index", "geom_face_split_tables", "geom_split_vertices_fwd_f32",
         "geom_split_vertices_bwd_f32")
EINVAL, ETOOBIG = _header.CONSTANTS["EINVAL"], _header.CONSTANTS["ETOOBIG"]


def test_the_new_symbols_are_declared_and_exported_and_the_abi_version_stands():
    L = _lib.lib()
    assert L.geom_abi_version() == 16 == _lib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout
    exported = {line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in "Tt"}
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in exported, name
        restype, argtypes = _header.PROTOTYPES[name]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p        # a code back, the stream last
    fields = [f for f, _ in _lib.FaceSplit._fields_]
    assert fields[:5] == ["nv", "nft", "nfa", "s", "nnz"] and len(fields) == 24 and _lib.FaceSplit is _header.STRUCTS["geom_face_split"]


def test_curvature_and_selection_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(nv=4, verts=P, nft=4, faces=P, nfa=4, face_list=P, curvature=P)
    call = lambda **kw: L.geom_face_curvature_f32(*{**ok, **kw}.values(), None)
    for size in ("nv", "nft", "nfa"):
        assert call(**{size: -1}) == EINVAL, size
    for pointer in ("verts", "faces", "face_list", "curvature"):
        assert call(**{pointer: None}) == EINVAL, pointer
    assert call(nfa=0, face_list=None, curvature=None) == 0                     # nothing to do
    assert L.geom_face_select_f32(-1, P, 70.0, P, P, None) == EINVAL
    assert L.geom_face_select_f32(4, None, 70.0, P, P, None) == EINVAL
    assert L.geom_face_select_f32(4, P, 70.0, None, P, None) == EINVAL
    assert L.geom_face_select_f32(4, P, 70.0, P, None, None) == EINVAL


def test_split_index_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(nv=4, nft=4, faces=P, nfa=4, face_list=P, s=2, splitting=P, corners=P, split_pos=P, unsplit_rank=P, face_s=P, inc_ptr=P,
              inc_item=P, cursor=P)
    call = lambda **kw: L.geom_face_split_index(*{**ok, **kw}.values(), None)
    for size in ("nv", "nft", "nfa", "s"):
        assert call(**{size: -1}) == EINVAL, size
    assert call(s=5) == EINVAL                                                  # more positions than active faces
    for pointer in [k for k, v in ok.items() if v == P]:
        assert call(**{pointer: None}) == EINVAL, pointer


def _tables(L, **kw):
    sizes = dict(nv=4, nft=4, nfa=4, s=1, nnz=16)
    args = _lib.FaceSplit(*[kw.pop(k, v) for k, v in sizes.items()], *[P] * 19)
    for name, value in kw.items():
        setattr(args, name, value)
    return L.geom_face_split_tables(ctypes.byref(args), None)


def test_split_tables_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.geom_face_split_tables(None, None) == EINVAL
    for size in ("nv", "nft", "nfa", "s", "nnz"):
        assert _tables(L, **{size: -1}) == EINVAL, size
    assert _tables(L, s=5) == EINVAL                                            # more faces to split than there are active ones
    assert _tables(L, nnz=2 ** 31 - 8, s=4) == ETOOBIG                          # the new CSR would not fit its int32 offsets
    for pointer in ("faces", "face_list", "corners", "split_pos", "unsplit_rank", "face_s", "inc_ptr", "inc_item", "rowptr", "col",
                    "new_faces", "new_face_list", "new_rowptr", "new_col", "new_val", "new_val_t", "new_ones"):
        assert _tables(L, **{pointer: None}) == EINVAL, pointer


@pytest.mark.parametrize("name", ["geom_split_vertices_fwd_f32", "geom_split_vertices_bwd_f32"])
def test_split_vertices_refuse_bad_arguments_before_any_launch(name):
    fn = getattr(_lib.lib(), name)
    for sizes in ((-1, 2, 8), (4, -1, 8), (4, 2, -1)):
        assert fn(*sizes, P, P, P, *((P,) if name.endswith("bwd_f32") else ()), P, P, None) == EINVAL, sizes
    slots = 6 if name.endswith("bwd_f32") else 5
    for missing in range(slots):
        ptrs = [P] * slots
        ptrs[missing] = None
        assert fn(4, 2, 8, *ptrs, None) == EINVAL, missing
    if name.endswith("fwd_f32"):
        assert fn(0, 2, 8, P, P, P, P, P, None) == EINVAL                       # new vertices of a mesh without vertices
        assert fn(0, 0, 8, None, None, None, None, None, None) == 0             # nothing to do
    else:
        assert fn(0, 0, 8, None, None, None, None, None, None, None) == 0


def test_split_info_refuses_a_wrong_number_and_calc_face_list_an_open_mesh():
    V, F = meshgen.icosphere(1)
    faces = torch.from_numpy(F)
    face_list = utils.calc_face_list(faces)                                     # (torch ops: runs where the faces are)
    assert face_list.shape == (80, 3, 3) and face_list.dtype == torch.int64
    fl = face_list.numpy()
    for i in (0, 17, 79):
        for j, (a, b) in enumerate(((0, 1), (1, 2), (0, 2))):
            nb, label, own = fl[i, j]
            assert own == i and nb != i and {F[i, a], F[i, b]} <= set(F[nb])
            la, lb = ((0, 1), (1, 2), (0, 2))[label]
            assert {F[nb, la], F[nb, lb]} == {F[i, a], F[i, b]}
    with pytest.raises(RuntimeError, match="exactly two faces"):
        utils.calc_face_list(faces[:-1])
    with pytest.raises(RuntimeError, match="exactly two faces"):
        utils.calc_face_list(torch.cat((faces, faces[:2])))                     # an edge shared by four faces
    info = {"faces": faces, "face_list": face_list, "adj_orig": torch.eye(42)}
    verts = torch.from_numpy(V)
    with pytest.raises(RuntimeError, match="number .* must be len"):
        utils.split_info(info, verts, verts, torch.tensor([3, 5]), 3)
    with pytest.raises(RuntimeError, match="HIP device"):                       # no CPU path
        utils.split_info(info, verts, verts, torch.tensor([3, 5]), 2)


def test_register_csr_hands_the_object_over_without_touching_the_tensor():
    adj = torch.eye(3)
    parts = (torch.tensor([0, 1, 2, 3], dtype=torch.int32), torch.tensor([0, 1, 2], dtype=torch.int32), torch.ones(3)) * 2
    csr = layers.register_csr(adj, parts)
    assert layers.registered_csr(adj) is csr and not hasattr(csr, "ell_w") and csr.rowptr is parts[0]
    assert layers.registered_csr(torch.eye(3)) is None
    adj.add_(1.0)                                                               # an in-place change drops the hand-over
    assert layers.registered_csr(adj) is None
