"""Shared by tests/test_ragged_split_gpu.py and tests/test_ragged_split_host.py: the union of five icospheres the ragged face
splitting (utils.ragged_calc_curve / ragged_split_info) is tested on, the restriction of a union to one of its meshes, and the two
thresholds, chosen on the CPU from the float64 restatement of the curvature."""
import functools
import types

import numpy as np
import torch

import face_split_helpers as fh
from geometrics_amd import meshgen, utils

LEVELS = (1, 2, 3, 1, 2)          # b = 5: 1050 vertices, 2080 faces -- five chunks of 256 vertices, nine of rows
SMOOTH = 3                        # the second icosphere(1) stays un-jittered: ties, and a regular surface
B = len(LEVELS)


def meshes(levels=LEVELS, smooth=SMOOTH):
    """[(verts fp32 [V,3], faces int64 [F,3])]: icospheres, each jittered under its own seed except `smooth`."""
    out = []
    for m, level in enumerate(levels):
        v, f = meshgen.icosphere(level)
        if m != smooth:
            v = meshgen.jittered_batch(v, 1, seed=41 + 10 * m)[0]
        out.append((np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64)))
    return out


def join(parts, shuffled, seed=7):
    """The union of [(verts, faces)] as numpy arrays: verts [Vt,3], faces [Ft,3] into it, vert_mesh [Vt].  shuffled: vertices
    and faces each permuted by a seeded permutation, the faces re-indexed -- the meshes interleave in both."""
    verts = np.concatenate([v for v, _ in parts])
    base = np.cumsum([0] + [len(v) for v, _ in parts])
    faces = np.concatenate([f + base[m] for m, (_, f) in enumerate(parts)])
    vert_mesh = np.concatenate([np.full(len(v), m, np.int64) for m, (v, _) in enumerate(parts)])
    if shuffled:
        rng = np.random.default_rng(seed)
        pv, pf = rng.permutation(len(verts)), rng.permutation(len(faces))
        new_id = np.empty(len(verts), np.int64)
        new_id[pv] = np.arange(len(verts))             # vertex pv[i] of the concatenation becomes vertex i
        verts, vert_mesh, faces = verts[pv], vert_mesh[pv], new_id[faces][pf]
    return types.SimpleNamespace(verts=np.ascontiguousarray(verts), faces=np.ascontiguousarray(faces), vert_mesh=vert_mesh,
                                 b=len(parts))


@functools.lru_cache(maxsize=None)
def union(shuffled):
    return join(meshes(), shuffled)


def rank_of(mask):
    """int64 [n]: the rank of every selected item among the selected ones, ascending; -1 elsewhere."""
    rank = np.full(len(mask), -1, np.int64)
    rank[mask] = np.arange(int(mask.sum()))
    return rank


def restrict(m, faces, face_list, face_mesh, vert_mesh):
    """The union's tables (numpy) restricted to mesh m and relabelled by rank inside the mesh -- vertices, faces and face_list
    rows each in ascending union index: (vids, fids, rows, faces_m, face_list_m).  vids / fids / rows: the union indices kept."""
    vmask, fmask = vert_mesh == m, face_mesh == m
    rmask = face_mesh[face_list[:, 0, 2]] == m
    vrank, frank = rank_of(vmask), rank_of(fmask)
    fl = face_list[rmask].copy()
    fl[:, :, 0], fl[:, :, 2] = frank[fl[:, :, 0]], frank[fl[:, :, 2]]
    faces_m = vrank[faces[fmask]]
    assert (faces_m >= 0).all() and (fl[:, :, (0, 2)] >= 0).all(), "mesh %d's faces or rows leave the mesh" % m
    return np.flatnonzero(vmask), np.flatnonzero(fmask), np.flatnonzero(rmask), faces_m, fl


def restrict_csr(vids, n, rowptr, col, *vals):
    """The rows `vids` of a CSR over n vertices with the columns relabelled by rank: (rowptr, col, *vals) of the mesh alone."""
    mask = np.zeros(n, bool)
    mask[vids] = True
    vrank = rank_of(mask)
    lens = (rowptr[1:] - rowptr[:-1])[vids]
    entries = np.concatenate([np.arange(rowptr[v], rowptr[v + 1]) for v in vids]) if len(vids) else np.zeros(0, np.int64)
    cols = vrank[col[entries]]
    assert (cols >= 0).all(), "a row of the mesh has a column outside the mesh"
    return (np.concatenate(([0], np.cumsum(lens))).astype(rowptr.dtype), cols.astype(col.dtype)) + tuple(v[entries] for v in vals)


def degrees64(verts, faces, face_list):
    """(degrees [Fa], margin [Fa]) in float64: the curvature of every active row in degrees and how far from a threshold it must
    stay for the fp32 decision (c * 180) / pi > angle to be the float64 one: the curvature's own bound (fh.curvature64) and the
    two roundings of the conversion, 3 * 2^-24 of the value with the rounding of pi."""
    c, bound = fh.curvature64(verts, faces, face_list)
    deg = np.degrees(c)
    return deg, np.degrees(bound) + 3.0 * fh.U * np.abs(deg)


def clear_of(angle, deg, margin):
    ok = ~np.isnan(deg)
    return bool((np.abs(deg[ok] - angle) > margin[ok]).all())


@functools.lru_cache(maxsize=None)
def angles():
    """(threshold, fallback): the lowest quarter degree at which EVERY mesh has at least 3 faces above it, and the lowest at which
    the un-jittered mesh has fewer than 3 and every other mesh still 3 -- no face of the union within its margin of either."""
    u = union(False)
    face_list = utils.calc_face_list(torch.from_numpy(u.faces)).numpy()
    deg, margin = degrees64(u.verts, u.faces, face_list)
    mesh = u.vert_mesh[u.faces[face_list[:, 0, 2], 0]]
    hits = lambda a: np.array([int((deg[mesh == m] > a).sum()) for m in range(u.b)])
    grid = np.arange(10.0, 40.0, 0.25)
    others = np.arange(u.b) != SMOOTH
    threshold = next(a for a in grid if clear_of(a, deg, margin) and (hits(a) >= 3).all() and hits(a)[SMOOTH] < (mesh == SMOOTH).sum())
    fallback = next(a for a in grid if clear_of(a, deg, margin) and hits(a)[SMOOTH] < 3 and (hits(a)[others] >= 3).all())
    return float(threshold), float(fallback)
