"""CPU: the entry points of the ragged face splitting (csrc/face_split.hip) are declared and exported and refuse bad arguments
with the header's codes before any launch (refusal paths only: nothing is launched here); utils.ragged_adj_init / ragged_calc_curve
/ ragged_split_info refuse what they document, naming the argument; calc_face_list serves a union as it stands."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import ragged_split_helpers as rh
from geometrics_amd import _header, _lib, layers, ragged, utils

P = 8        # any non-null address: validation never dereferences
EINVAL, ETOOBIG = _header.CONSTANTS["EINVAL"], _header.CONSTANTS["ETOOBIG"]
NAMES = ("geom_face_select_ragged_f32", "geom_face_split_index_ragged")


def test_the_new_symbols_resolve_through_the_header_derived_binding():
    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout
    exported = {line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in "Tt"}
    for name in NAMES + ("geom_face_split_index_ragged_words",):
        assert name in _lib.declared_symbols() and name in exported and getattr(L, name).argtypes is not None, name
    for name in NAMES:
        restype, argtypes = _header.PROTOTYPES[name]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p        # a code back, the stream last
    assert _header.PROTOTYPES["geom_face_split_index_ragged_words"][0] is ctypes.c_int64
    assert len(_header.STRUCTS["geom_face_split"]._fields_) == 24                 # no new field for the ids


def test_the_ragged_selection_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(nfa=4, curvature=P, angle=70.0, b=2, row_list=P, row_off=P, stats=P, selected=P, counts=P, totals=P)
    call = lambda **kw: L.geom_face_select_ragged_f32(*{**ok, **kw}.values(), None)
    for size in ("nfa", "b"):
        assert call(**{size: -1}) == EINVAL, size
    for pointer in [k for k, v in ok.items() if v == P]:
        assert call(**{pointer: None}) == EINVAL, pointer


def test_the_ragged_split_index_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(nv=4, nft=4, faces=P, nfa=4, face_list=P, s=2, splitting=P, vert_mesh=P, face_mesh=P, corners=P, split_pos=P,
              unsplit_rank=P, face_s=P, inc_ptr=P, inc_item=P, vert_mesh_new=P, face_mesh_new=P, workspace=P)
    call = lambda **kw: L.geom_face_split_index_ragged(*{**ok, **kw}.values(), None)
    for size in ("nv", "nft", "nfa", "s"):
        assert call(**{size: -1}) == EINVAL, size
    assert call(s=5) == EINVAL                                                  # more positions than active faces
    for pointer in [k for k, v in ok.items() if v == P]:
        assert call(**{pointer: None}) == EINVAL, pointer
    big = 2 ** 31 - 8
    assert call(nfa=big, s=big // 2) == ETOOBIG                                 # 3 s no longer fits the tables' int32 sizes
    words = L.geom_face_split_index_ragged_words
    assert words(-1, 4, 4, 2) == words(4, -1, 4, 2) == words(4, 4, -1, 2) == words(4, 4, 4, -1) == EINVAL
    # per vertex a count, per chunk of 256 vertices and of 256 rows a total, per row and per face a mark, per corner a place
    assert words(1050, 2080, 2080, 100) == 1050 + 5 + 9 + 2080 + 2080 + 300 and words(0, 0, 0, 0) == 0


def small_info():
    u = rh.join(rh.meshes((1, 1), smooth=1), shuffled=True)
    return u, utils.ragged_adj_init(torch.from_numpy(u.faces), torch.from_numpy(u.vert_mesh), u.b)


def test_calc_face_list_serves_a_union_as_it_stands_and_the_info_has_no_dense_matrix():
    u, info = small_info()
    assert sorted(info) == ["b", "csr", "face_list", "face_mesh", "faces", "vert_mesh"] and info["b"] == 2
    assert isinstance(info["csr"], layers._Csr) and info["csr"].nv == len(u.verts) == 84
    assert info["face_mesh"].dtype == torch.int64 and torch.equal(info["face_mesh"], ragged.face_mesh(info["faces"], info["vert_mesh"]))
    tables = tuple(info[k].numpy() for k in ("faces", "face_list", "face_mesh", "vert_mesh"))
    for m in range(u.b):     # an edge is still shared by exactly two faces, both of its own mesh: the union's list is each mesh's
        _, _, rows, faces_m, fl_m = rh.restrict(m, *tables)
        assert len(rows) == 80 and np.array_equal(fl_m, utils.calc_face_list(torch.from_numpy(faces_m)).numpy())
    faces, face_mesh = utils.ragged_active_faces(info)
    assert utils.ragged_active_faces(info)[1] is face_mesh and torch.equal(faces, info["faces"]) and torch.equal(face_mesh, info["face_mesh"])
    row_list, row_off = ragged.group_rows(info["face_list"], info["face_mesh"], 2)
    assert row_off.tolist() == [0, 80, 160] and row_list.dtype == torch.int32
    assert torch.equal(row_list[:80].long(), torch.from_numpy(np.flatnonzero(tables[2] == 0)))


def test_the_python_argument_checks_name_the_argument():
    u, info = small_info()
    faces, vert_mesh = torch.from_numpy(u.faces), torch.from_numpy(u.vert_mesh)
    verts, features = torch.from_numpy(u.verts), torch.zeros(len(u.verts), 4)
    with pytest.raises(RuntimeError, match=r"faces must be an \[Ft,3\] int64"):
        utils.ragged_adj_init(faces.reshape(-1, 2), vert_mesh, 2)
    with pytest.raises(RuntimeError, match="vert_mesh must be a one-dimensional int64"):
        utils.ragged_adj_init(faces, vert_mesh.to(torch.int32), 2)
    split = lambda verts=verts, features=features, positions=torch.tensor([3, 5]), **kw: utils.ragged_split_info(
        {**info, **kw}, verts, features, positions)
    with pytest.raises(RuntimeError, match=r"info\['faces'\] must be \[Ft,3\]"):
        split(faces=faces.reshape(-1, 2))
    with pytest.raises(RuntimeError, match=r"info\['face_mesh'\] must be int64 \[160\]"):
        split(face_mesh=info["face_mesh"].to(torch.int32))
    with pytest.raises(RuntimeError, match=r"info\['face_mesh'\] must be int64 \[160\]"):
        split(face_mesh=info["face_mesh"][:-1])
    with pytest.raises(RuntimeError, match=r"info\['vert_mesh'\] must be int64 \[84\]"):
        split(vert_mesh=vert_mesh.to(torch.int32))
    with pytest.raises(RuntimeError, match=r"info\['vert_mesh'\] must be int64 \[84\]"):
        split(vert_mesh=vert_mesh[:-1])
    with pytest.raises(RuntimeError, match="features .* must have the 84 rows of verts"):
        split(features=features[:-1])
    with pytest.raises(RuntimeError, match="splitting holds 161 positions for 160 active faces"):
        split(positions=torch.arange(161))
    with pytest.raises(RuntimeError, match=r"info\['csr'\] must be the union's adjacency"):
        split(csr=None)
    with pytest.raises(RuntimeError, match=r"info\['face_mesh'\] must be int64"):
        utils.ragged_calc_curve(verts, {**info, "face_mesh": info["face_mesh"].to(torch.int32)})
    with pytest.raises(RuntimeError, match="HIP device"):                       # no CPU path
        split()
