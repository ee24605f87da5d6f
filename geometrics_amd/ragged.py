"""Ragged batches of meshes for the auto-encoder path.

The reference encodes a batch one mesh at a time -- `for mesh, adj in zip(batch['verts'], batch['adjs'])`
(auto_encoder.py:71-76) -- because every ShapeNet mesh has its own vertex count and its own dense
normalised adjacency (utils.py:251-258).  On MI355X that is ~17 x 5 small launches per mesh.  Here the
meshes are concatenated along the vertex axis and their adjacencies become ONE block-diagonal CSR, so a
0N-GCN layer over the whole batch is one GEMM over sum(V) rows plus one aggregation launch, and GCNMax's
per-mesh maximum is a segmented reduction (csrc/segment.hip).
"""
import torch

from . import layers
from ._identity import ByTensor


class RaggedMeshBatch:
    """verts [sum(V),3] fp32, offsets [B+1] int64 (device), sizes (host), csr = block-diagonal normalised
    adjacency in the layout the 0N-GCN kernels consume (pass it wherever a layer takes `adj`)."""

    def __init__(self, verts, sizes, csr):
        self.verts = verts
        self.sizes = [int(s) for s in sizes]
        self.num_meshes = len(self.sizes)
        self.max_len = max(self.sizes) if self.sizes else 0
        host = torch.tensor([0] + self.sizes, dtype=torch.int64).cumsum(0)
        self.total = int(host[-1])
        self.offsets = host.to(verts.device)
        self.csr = csr

    # ---------------------------------------------------------------- builders ----
    @classmethod
    def from_faces(cls, verts_list, faces_list):
        """Straight from the triangle lists: the normalised adjacency D^-1 (A + I) of utils.py:96-131 per mesh,
        assembled directly in CSR -- no dense [V,V] matrix is ever formed and there is one host sync (the
        number of distinct edges) for the whole batch."""
        if len(verts_list) != len(faces_list) or not verts_list:
            raise RuntimeError("need one face list per mesh and at least one mesh")
        dev = verts_list[0].device
        if dev.type != "cuda":
            raise RuntimeError("ragged batches live on a HIP device; geometrics_amd has no CPU path")
        sizes = [int(v.shape[0]) for v in verts_list]
        total = sum(sizes)
        base, shifted = 0, []
        for v, f in zip(verts_list, faces_list):
            if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
                raise RuntimeError("meshes are (verts [V,3], faces [F,3]) pairs")
            shifted.append(f.to(dev, torch.int64) + base)
            base += v.shape[0]
        csr = csr_from_faces(torch.cat(shifted), total)
        verts = torch.cat([v.to(dev, torch.float32) for v in verts_list]).contiguous()
        return cls(verts, sizes, csr)

    @classmethod
    def from_dense(cls, verts_list, adjs_list):
        """From the per-mesh dense adjacencies the reference's data loader hands over (`batch['adjs']`,
        utils.py:256-257).  Values are taken as they are (any normalisation)."""
        if len(verts_list) != len(adjs_list) or not verts_list:
            raise RuntimeError("need one adjacency per mesh and at least one mesh")
        dev = verts_list[0].device
        if dev.type != "cuda":
            raise RuntimeError("ragged batches live on a HIP device; geometrics_amd has no CPU path")
        parts, parts_t, base = [], [], 0
        for v, adj in zip(verts_list, adjs_list):
            if adj.shape != (v.shape[0], v.shape[0]):
                raise RuntimeError("adjacency %s does not match %d vertices" % (tuple(adj.shape), v.shape[0]))
            dense = adj.detach().to(dev, torch.float32)
            parts.append(layers._to_csr(dense) + (base,))
            parts_t.append(layers._to_csr(dense.t()) + (base,))
            base += v.shape[0]

        def join(ps):
            nnz_base, rowptrs, cols, vals = 0, [torch.zeros(1, dtype=torch.int32, device=dev)], [], []
            for rowptr, col, val, vbase in ps:
                rowptrs.append(rowptr[1:] + nnz_base)
                cols.append(col + vbase)
                vals.append(val)
                nnz_base += int(col.numel())
            return torch.cat(rowptrs).contiguous(), torch.cat(cols).contiguous(), torch.cat(vals).contiguous()

        csr = layers.csr_from_parts(*join(parts), *join(parts_t))
        verts = torch.cat([v.to(dev, torch.float32) for v in verts_list]).contiguous()
        return cls(verts, [v.shape[0] for v in verts_list], csr)

    # ------------------------------------------------------------------ helpers ----
    def split(self, x):
        """[sum(V), ...] -> list of per-mesh views."""
        return list(torch.split(x, self.sizes, dim=0))


# ------------------------------------------------- ragged batches of meshes with their OWN faces (the surface loss) ----
# After the first adaptive split every image of a batch owns a topology.  The batch is then ONE union mesh -- vertices
# concatenated as above, faces [Ft,3] indexing the union -- plus the id of its mesh per face.  The two searches of the surface
# loss must not cross from one mesh into another, so they walk the faces GROUPED by mesh.
_group_cache = ByTensor()    # (faces, face_mesh) or (face_mesh,), extra: the mesh count -> (face_list, face_off)
_vertex_group_cache = ByTensor()    # (vert_mesh,), extra: the mesh count -> (vert_list, vert_off)


def _group_by_mesh(ids, b):
    """(list int32 [n], off int32 [b+1]) of int64 mesh ids: the items grouped by id, in their own order inside a group (a stable
    argsort), and the first position whose id is >= m for m = 0 ... b (a binary search over the sorted ids, which unlike
    bincount needs no host read).  The one statement of the construction group_faces and group_vertices hand out."""
    order = torch.argsort(ids, stable=True)
    bounds = torch.arange(int(b) + 1, dtype=torch.int64, device=ids.device)
    off = torch.searchsorted(ids[order].contiguous(), bounds)      # first position whose id is >= m
    return order.to(torch.int32).contiguous(), off.to(torch.int32).contiguous()


def group_faces(face_mesh, b, faces=None):
    """(face_list int32 [Ft], face_off int32 [b+1]) on face_mesh's device: face_list = argsort(face_mesh, stable=True), the
    faces grouped by mesh and ascending inside a mesh; face_off = [0, cumsum(bincount(face_mesh, minlength=b))], where each
    group starts.  Position k of mesh m is the face face_list[face_off[m] + k].  Torch ops only, no host read (the counts
    come from a binary search over the sorted ids, which unlike bincount needs none); a face whose id is outside [0, b)
    belongs to no mesh.  Cached per (faces, face_mesh) TENSOR OBJECTS and their in-place versions, as utils.active_faces."""
    if face_mesh.dim() != 1:
        raise RuntimeError("face_mesh must be [Ft] (got shape %s)" % (tuple(face_mesh.shape),))
    keys = (face_mesh,) if faces is None else (faces, face_mesh)
    hit = _group_cache.get(*keys, extra=int(b))
    if hit is None:
        with torch.no_grad():
            hit = _group_cache.put(_group_by_mesh(face_mesh.detach().to(torch.int64), b), *keys, extra=int(b))
    return hit


_position_cache = ByTensor()    # the keys of group_faces, extra: the mesh count -> face_pos


def face_positions(face_mesh, b, faces=None):
    """face_pos int32 [Ft] on face_mesh's device: the inverse permutation of group_faces' face_list -- face f stands at
    face_list[face_pos[f]], so its position inside its mesh m is face_pos[f] - face_off[m] -- with -1 for a face of no mesh (an
    id outside [0, b)).  What the ordered backward of the ragged surface loss bins by (ops.RaggedSurfaceLoss).  Torch ops
    only, no host read; cached per tensor objects like group_faces."""
    keys = (face_mesh,) if faces is None else (faces, face_mesh)
    hit = _position_cache.get(*keys, extra=int(b))
    if hit is None:
        face_list, _ = group_faces(face_mesh, b, faces)
        with torch.no_grad():
            ids = face_mesh.detach().to(torch.int64)
            pos = torch.empty_like(face_list)
            pos[face_list.to(torch.int64)] = torch.arange(face_list.numel(), dtype=torch.int32, device=face_list.device)
            pos = torch.where((ids >= 0) & (ids < int(b)), pos, torch.full_like(pos, -1))
        hit = _position_cache.put(pos.contiguous(), *keys, extra=int(b))
    return hit


_vertex_face_cache = ByTensor()    # (faces,), extra: the vertex count -> (vf_ptr, vf_item)


def vertex_faces(faces, nv):
    """(vf_ptr int32 [nv+1], vf_item int32 [3 Ft]) of ops.vertex_faces -- vertex -> incident (face << 2 | corner), ascending per
    vertex: what the gather backward walks -- built WITHOUT its two host reads: a stable argsort of the flattened corners, and
    the row starts by a binary search over arange(nv + 1) (the construction of group_faces).  A corner outside [0, nv) falls in
    front of vf_ptr[0] or behind vf_ptr[nv] and is never walked.  A ragged stage gets new faces after every split, so this table
    is rebuilt every step: a host read here would be the only one of the loss.  Cached per faces TENSOR OBJECT and version."""
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64:
        raise RuntimeError("faces must be [Ft,3] int64 (got %s %s)" % (faces.dtype, tuple(faces.shape)))
    hit = _vertex_face_cache.get(faces, extra=int(nv))
    if hit is None:
        with torch.no_grad():
            flat = faces.detach().reshape(-1)
            order = torch.argsort(flat, stable=True)                      # position p = 3*face + corner
            vf_item = (((order // 3) << 2) | (order % 3)).to(torch.int32).contiguous()
            bounds = torch.arange(int(nv) + 1, dtype=torch.int64, device=faces.device)
            vf_ptr = torch.searchsorted(flat[order].contiguous(), bounds).to(torch.int32).contiguous()
        hit = _vertex_face_cache.put((vf_ptr, vf_item), faces, extra=int(nv))
    return hit


def group_vertices(vert_mesh, b):
    """(vert_list int32 [Vt], vert_off int32 [b+1]) on vert_mesh's device, for the ragged pooling: the
    union's vertices grouped by mesh -- a stable argsort of the ids clamped to [-1, b], so a vertex of no mesh stands in front of
    mesh 0's group or behind the last one's -- and where each group starts: position k of mesh m is the vertex
    vert_list[vert_off[m] + k], and [vert_off[0], vert_off[b]) are the vertices that belong to a mesh.  The construction of
    group_faces: no host read, cached per vert_mesh TENSOR OBJECT and in-place version."""
    if vert_mesh.dim() != 1 or vert_mesh.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("vert_mesh must be a one-dimensional int32 or int64 tensor (got %s %s)" % (vert_mesh.dtype, tuple(vert_mesh.shape)))
    hit = _vertex_group_cache.get(vert_mesh, extra=int(b))
    if hit is None:
        with torch.no_grad():
            ids = vert_mesh.detach().to(torch.int64).clamp(-1, int(b))
            hit = _vertex_group_cache.put(_group_by_mesh(ids, b), vert_mesh, extra=int(b))
    return hit


_row_group_cache = ByTensor()    # (face_list, face_mesh), extra: the mesh count -> (row_list, row_off)


def group_rows(face_list, face_mesh, b):
    """(row_list int32 [Fa], row_off int32 [b+1]) for utils.ragged_calc_curve: the ACTIVE rows of a union's face_list [Fa,3,3]
    grouped by the mesh of their face, face_mesh[face_list[i, 0, 2]], ascending inside a mesh; rows whose id is outside [0, b)
    stand in front of row_off[0] or behind row_off[b].  The construction of group_faces on the rows' ids: no host read, cached
    per face_list and face_mesh TENSOR OBJECTS and their in-place versions."""
    if face_list.dim() != 3 or face_list.shape[1:] != (3, 3):
        raise RuntimeError("face_list must be [Fa,3,3] (got shape %s)" % (tuple(face_list.shape),))
    if face_mesh.dim() != 1 or face_mesh.dtype != torch.int64:
        raise RuntimeError("face_mesh must be a one-dimensional int64 tensor (got %s %s)" % (face_mesh.dtype, tuple(face_mesh.shape)))
    hit = _row_group_cache.get(face_list, face_mesh, extra=int(b))
    if hit is None:
        with torch.no_grad():
            ids = face_mesh.detach().index_select(0, face_list[:, 0, 2]).clamp(-1, int(b))
            hit = _row_group_cache.put(_group_by_mesh(ids, b), face_list, face_mesh, extra=int(b))
    return hit


def face_mesh(faces, vert_mesh):
    """vert_mesh[faces[:, 0]]: the mesh of every face from the mesh of every vertex -- for callers that track ids per vertex
    (through utils.split_info a new vertex inherits its face's mesh)."""
    return vert_mesh[faces[:, 0]]


def csr_from_faces(faces, nv):
    """The adjacency of a union mesh straight from its triangles: faces [Ft,3] int64 into nv vertices -> a layers._Csr of the
    binary pattern with self loops, block-diagonal wherever no face joins two meshes; its values are the normalised adjacency
    D^-1 (A + I) of utils.py:96-131 (pass it wherever a layer takes `adj`), its rowptr / col / inv_deg are what the Laplacian
    and utils.ragged_stage_regularisers read.  Assembled directly in CSR: no dense [V,V] matrix is ever formed and the number
    of distinct edges is the one host read of the assembly (layers' derived tables look at the row lengths once more); build
    it once per topology and keep the result."""
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64:
        raise RuntimeError("faces must be [Ft,3] int64 (got %s %s)" % (faces.dtype, tuple(faces.shape)))
    total, dev = int(nv), faces.device
    with torch.no_grad():
        a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
        loops = torch.arange(total, device=dev)
        rows = torch.cat([a, a, b, b, c, c, loops])
        cols = torch.cat([b, c, a, c, a, b, loops])
        keys = torch.unique(rows * total + cols)          # sorted: row-major == CSR order
        rows, cols = keys // total, keys % total
        # where each row starts: a search over the sorted rows (bincount would read its maximum on the host)
        rowptr = torch.searchsorted(rows.contiguous(), torch.arange(total + 1, device=dev))
        counts = rowptr[1:] - rowptr[:-1]
        r_inv = 1.0 / counts.to(torch.float32)            # normalize_adj: 1 / row sum of the binary matrix
        rowptr, col = rowptr.to(torch.int32), cols.to(torch.int32).contiguous()
        # the pattern is symmetric, so CSR^T shares rowptr/col and only swaps which row's scale an entry carries
        return layers.csr_from_parts(rowptr, col, r_inv[rows].contiguous(), rowptr, col, r_inv[cols].contiguous())


_count_cache = ByTensor()    # (ids,), extra: the mesh count -> (ids int32, counts int64 [b])


def mesh_counts(ids, b):
    """(ids as int32 [n], counts int64 [b]) on ids' device: how many vertices (or faces) every mesh of [0, b) holds.  An id
    outside [0, b) belongs to no mesh and is counted nowhere (it is stored as -1 or b).  A sort and a binary search, no host
    read (bincount needs one); cached per ids TENSOR OBJECT and in-place version, as group_faces."""
    if ids.dim() != 1 or ids.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("mesh ids must be a one-dimensional int32 or int64 tensor (got %s %s)" % (ids.dtype, tuple(ids.shape)))
    hit = _count_cache.get(ids, extra=int(b))
    if hit is None:
        with torch.no_grad():
            clamped = ids.detach().to(torch.int64).clamp(-1, int(b))
            bounds = torch.arange(int(b) + 1, dtype=torch.int64, device=ids.device)
            starts = torch.searchsorted(torch.sort(clamped).values, bounds)      # first position whose id is >= m
            hit = _count_cache.put((clamped.to(torch.int32).contiguous(), (starts[1:] - starts[:-1]).contiguous()), ids, extra=int(b))
    return hit


_coef_cache = ByTensor()     # the id tensors and the weight tensors, extra: (b, the python weights, ...) -> coef [3,b]


def _weight_row(w, b, dev):
    if torch.is_tensor(w):
        if w.shape != (b,) or w.dtype != torch.float32 or w.device != dev:
            raise RuntimeError("a per-mesh weight must be a [%d] float32 tensor on %s (got %s %s on %s)"
                               % (b, dev, w.dtype, tuple(w.shape), w.device))
        return w.detach().to(torch.float64)
    return torch.full((b,), float(w), dtype=torch.float64, device=dev)


def regulariser_coefficients(vert_counts, face_counts, b, w_lap, w_move, w_edge):
    """coef [3,b] fp32 of the ragged stage regularisers from the per-mesh counts (int64 [b] each, on their device; vert_counts
    None: no Laplacian and no displacement term): rows w_lap[m] / (b V_m), w_move[m] / (b V_m), w_edge[m] / (3 b F_m), formed in
    float64 and rounded once.  A weight is a python float or a [b] fp32 tensor.  The reference's mean over nothing is NaN: a
    mesh without a vertex gets NaN in the first two rows WHATEVER its weights, a mesh without a face NaN in the third where
    its edge weight is not 0 (and 0 where it is).  Torch ops on the counts' device, no host read."""
    dev = face_counts.device
    nan = torch.full((b,), float("nan"), dtype=torch.float64, device=dev)
    zero = torch.zeros(b, dtype=torch.float64, device=dev)
    if vert_counts is None:
        lap = move = zero
    else:
        per_mesh = b * vert_counts.to(torch.float64)
        lap, move = (torch.where(vert_counts == 0, nan, torch.where(w == 0, zero, w / per_mesh))
                     for w in (_weight_row(w_lap, b, dev), _weight_row(w_move, b, dev)))
    w = _weight_row(w_edge, b, dev)
    edge = torch.where(w == 0, zero, torch.where(face_counts == 0, nan, w / (3.0 * b * face_counts.to(torch.float64))))
    return torch.stack((lap, move, edge)).to(torch.float32).contiguous()


def regulariser_tables(face_mesh, vert_mesh, b, w_lap, w_move, w_edge):
    """(face_mesh int32, vert_mesh int32 or None, coef [3,b]) for ops.RaggedStageRegularisers; vert_mesh None: the edge term
    alone.  The table is cached per id and weight TENSOR OBJECTS (and their in-place versions), the mesh count and the python
    weights: a training step rebuilds nothing."""
    b = int(b)
    weights = (w_lap, w_move, w_edge)
    keys = [t for t in (face_mesh, vert_mesh) + weights if torch.is_tensor(t)]
    extra = (b, vert_mesh is None) + tuple(None if torch.is_tensor(w) else float(w) for w in weights)
    hit = _coef_cache.get(*keys, extra=extra)
    if hit is None:
        with torch.no_grad():
            fm, face_counts = mesh_counts(face_mesh, b)
            vm, vert_counts = (None, None) if vert_mesh is None else mesh_counts(vert_mesh, b)
            hit = _coef_cache.put((fm, vm, regulariser_coefficients(vert_counts, face_counts, b, *weights)), *keys, extra=extra)
    return hit


__all__ = ["RaggedMeshBatch", "group_faces", "face_positions", "vertex_faces", "group_vertices", "group_rows", "face_mesh", "csr_from_faces", "mesh_counts", "regulariser_coefficients",
           "regulariser_tables"]
