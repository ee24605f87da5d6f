"""Loss / sampling / adjacency helpers with the reference's names and call signatures
(reference utils.py:95-131, 393-662), running on the HIP kernels of libgeom_hip.so.

What changes underneath (never in results beyond fp32 round-off, NN indices bit-exact):
  * batch_sample: one fused gather+barycentric kernel and batched random draws instead of
    ~20 eager ops and a python loop of B multinomials;
  * the Chamfer term reuses the squared distances the NN scan already computed;
  * the three [B,F,3] corner gathers feeding tri_dist are done inside the scan kernel;
  * calc_point_to_line evaluates only the selected candidate (no seven boolean-mask
    scatters, each of which is a host sync in the reference) and has an analytic backward;
  * no host synchronisation unless f1=True (the reference syncs on every call through the
    dead `ratio = dist_1.cpu()/dist_2.cpu()` line, utils.py:482).
"""
import math

import torch

from . import ops
from ._identity import ByTensor
from .encoder import latent_loss  # noqa: F401  (GEOMetrics.py:165-171 on two kernels, no host read)
from .chamfer_distance import ChamferDistance
from .tri_distance import TriDistance

chamfer_dist = ChamferDistance()
tri_dist = TriDistance()

LOSS_SCALE = 3000.0      # reference utils.py:420, 484
F1_SCALE = 0.57          # reference utils.py:425-426
F1_THRESHOLD = 1e-2      # reference utils.py:430-431


# ------------------------------------------------------------------ adjacency ----
def calc_adj(faces):
    """Dense binary adjacency with self loops (reference utils.py:115-131)."""
    n = int(faces.max()) + 1
    adj = torch.eye(n, device=faces.device)
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    rows = torch.cat([a, a, b, b, c, c])
    cols = torch.cat([b, c, a, c, a, b])
    adj[rows, cols] = 1
    return adj


def normalize_adj(mx):
    """D^-1 (A+I): rows sum to 1 (reference utils.py:96-101; a row scaling is bit-identical to
    the reference's product with a diagonal matrix and skips its V^3 flops)."""
    r_inv = (1.0 / mx.sum(1)).view(-1)
    r_inv[r_inv != r_inv] = 0.0
    return mx * r_inv.unsqueeze(1)


def adj_init(faces):
    """{'adj': normalised, 'adj_orig': binary, 'faces': faces} (reference utils.py:104-113)."""
    adj_orig = calc_adj(faces)
    return {"adj": normalize_adj(adj_orig.clone()), "adj_orig": adj_orig, "faces": faces}


# ------------------------------------- adaptive face splitting (old_GEOMetrics/utils.py) ----
def calc_face_list(faces):
    """int64 [F,3,3] on the device: row i, slot j = [the face across edge j, the label that face gives the shared edge, i], edges
    0 / 1 / 2 = the vertex pairs (0,1), (1,2), (0,2) (reference old_GEOMetrics/utils.py:158-179, an O(F^2) python loop there;
    here one sort of the 3F edge keys).  Set-up code on torch ops, one host read (the check).  An edge that is not shared by
    exactly two faces raises -- the reference silently returns a ragged list for such a mesh.  The UNION of a ragged batch
    (faces of several meshes indexing their concatenated vertices, in any order) is such a mesh as it stands: no edge joins two
    meshes, so every edge is still shared by exactly two faces, both of its own mesh (ragged_adj_init)."""
    faces = torch.as_tensor(faces)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("faces must be [F,3] (got shape %s)" % (tuple(faces.shape),))
    faces = faces.to(torch.int64)
    nf = faces.shape[0]
    a = torch.stack((faces[:, 0], faces[:, 1], faces[:, 0]), dim=1)          # edge j of face i: (a, b)[i, j]
    b = torch.stack((faces[:, 1], faces[:, 2], faces[:, 2]), dim=1)
    span = faces.max() + 1 if nf else 1
    keys = (torch.minimum(a, b) * span + torch.maximum(a, b)).reshape(-1)    # entry 3 i + j
    order = torch.argsort(keys, stable=True)
    sorted_keys = keys[order]
    paired = nf > 0 and (3 * nf) % 2 == 0
    if paired:
        first, second = sorted_keys[0::2], sorted_keys[1::2]
        paired = bool((first == second).all() & (first[1:] != second[:-1]).all())
    if not paired:
        raise RuntimeError("calc_face_list: every edge must be shared by exactly two faces (a closed manifold triangle mesh)")
    partner = torch.empty_like(order)
    partner[order[0::2]] = order[1::2]
    partner[order[1::2]] = order[0::2]
    own = torch.arange(nf, device=faces.device).repeat_interleave(3)
    return torch.stack((torch.div(partner, 3, rounding_mode="floor"), partner % 3, own), dim=1).reshape(nf, 3, 3).contiguous()


_active_cache = ByTensor()   # (face_list, faces) -> the active faces


def active_faces(info):
    """info['faces'][info['face_list'][:, 0, 2]]: the faces the losses run on after a split (the reference's calc_edge and its
    driver take them the same way, old_GEOMetrics/utils.py:674-677).  Cached per face_list and faces TENSOR OBJECTS and their
    in-place versions (_identity.ByTensor): every loss call on a split mesh passes the same tensor as 'faces', so the tables
    keyed on that tensor are built once."""
    face_list, faces = info["face_list"], info["faces"]
    active = _active_cache.get(face_list, faces)
    if active is None:
        with torch.no_grad():
            active = _active_cache.put(faces.index_select(0, face_list[:, 0, 2]).contiguous(), face_list, faces)
    return active


def calc_curve(verts, info, angle=70):
    """Positions into info['face_list'] of the faces whose mean dihedral angle to their three neighbours exceeds `angle` degrees,
    ascending (reference old_GEOMetrics/utils.py:431-473); fewer than 3 such faces: the 3 faces of largest curvature, largest
    first (the reference's topk(sorted=False) leaves their order open).  A face with a zero-area face among itself and its
    neighbours has curvature NaN and is never selected.  Two launches and ONE host read (the count, which the size of the
    result depends on).  Not differentiable: the result is indices."""
    curvature = ops.face_curvature(verts, info["faces"], info["face_list"])
    selected, count_top3 = ops.select_faces(curvature, angle)
    count, *top3 = count_top3.tolist()                 # the one host read
    if count < 3:
        if min(top3) < 0:
            raise RuntimeError("calc_curve: fewer than 3 faces have a curvature (degenerate or too small a mesh)")
        return count_top3[1:].clone()
    return selected[:count]


def split_info(info, verts, features, splitting, number):
    """Split the active faces at positions `splitting` of info['face_list'] (reference old_GEOMetrics/utils.py:481-634): a
    vertex at each such face's centre -- position and features the mean (x/3 + y/3) + z/3 of its corners --, the face replaced
    by its three children (x,y,n), (n,y,z), (x,n,z).  Returns (new_info, new_verts [V+S,3], new_features [V+S,C]); new_info has
    'adj' (normalised) and 'adj_orig' (binary), dense fp32 [V+S,V+S] on the device, 'faces' int64 [Ft+3S,3] (the split faces
    stay in it, dead) and 'face_list' int64 [Fa+2S,3,3] -- rows and every index exactly the reference's: the unsplit rows in
    their old order, then the S first, S second and S third children.  Differentiable in verts and features.
      * `number` must equal len(splitting) (the reference takes both and trusts them);
      * `splitting` must hold UNIQUE positions in [0, Fa): not checked -- checking would need a host read, and this function
        makes none (info['adj_orig'] not yet seen by the layers is read once, as for any adjacency);
      * the dense matrices are filled from the CSR of the new adjacency, which is handed to the layers at the same time
        (layers.register_csr): adjacency_csr(new_info['adj'] / ['adj_orig']) never reads the matrices back."""
    from . import layers
    splitting = torch.as_tensor(splitting, device=verts.device).to(torch.int64).reshape(-1).contiguous()
    if int(number) != splitting.numel():
        raise RuntimeError("split_info: number (%d) must be len(splitting) (%d)" % (int(number), splitting.numel()))
    faces = ops._lib.require(info["faces"], "info['faces']", torch.int64, 2, 3)
    face_list = ops._lib.require(info["face_list"], "info['face_list']", torch.int64, 3, 3)
    if face_list.shape[1] != 3:
        raise RuntimeError("info['face_list'] must be [Fa,3,3] (got shape %s)" % (tuple(face_list.shape),))
    if splitting.numel() > face_list.shape[0]:
        raise RuntimeError("split_info: %d positions for %d active faces" % (splitting.numel(), face_list.shape[0]))
    nv = verts.shape[0]
    old = layers.registered_csr(info["adj_orig"]) or layers.adjacency_csr(info["adj_orig"])
    if not getattr(old, "symmetric_structure", True):      # (a CSR this function handed over is symmetric by construction)
        raise RuntimeError("info['adj_orig'] must have a symmetric pattern")
    if old.rowptr.numel() != nv + 1:
        raise RuntimeError("info['adj_orig'] is %d x %d but verts has %d rows" % (old.rowptr.numel() - 1, old.rowptr.numel() - 1, nv))
    ix = ops.split_index(faces, face_list, splitting, nv)
    t = ops.split_tables(faces, face_list, ix, old.rowptr, old.col)
    new_verts, new_features = ops.SplitVertices.apply(verts, features, ix)
    # the pattern is symmetric: it is its own transpose; the normalised matrix's transpose has the columns' 1 / row length
    layers.register_csr(t["adj"], (t["rowptr"], t["col"], t["val"], t["rowptr"], t["col"], t["val_t"]))
    layers.register_csr(t["adj_orig"], (t["rowptr"], t["col"], t["ones"], t["rowptr"], t["col"], t["ones"]))
    new_info = {"adj": t["adj"], "adj_orig": t["adj_orig"], "faces": t["new_faces"], "face_list": t["new_face_list"]}
    return new_info, new_verts, new_features


# ------------------------------------- the same for a ragged batch held as ONE union mesh ----
def _ragged_info(info, nv=None):
    """The checked tables of a union's info: (faces, face_list, face_mesh, vert_mesh, b).  Shapes and dtypes first (they need no
    device), each complaint naming its argument."""
    faces, face_list, face_mesh, vert_mesh = info["faces"], info["face_list"], info["face_mesh"], info["vert_mesh"]
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64:
        raise RuntimeError("info['faces'] must be [Ft,3] int64 (got %s %s)" % (faces.dtype, tuple(faces.shape)))
    if face_list.dim() != 3 or face_list.shape[1:] != (3, 3) or face_list.dtype != torch.int64:
        raise RuntimeError("info['face_list'] must be [Fa,3,3] int64 (got %s %s)" % (face_list.dtype, tuple(face_list.shape)))
    if face_mesh.dtype != torch.int64 or face_mesh.shape != (faces.shape[0],):
        raise RuntimeError("info['face_mesh'] must be int64 [%d], one id per face ever made (got %s %s)"
                           % (faces.shape[0], face_mesh.dtype, tuple(face_mesh.shape)))
    if vert_mesh.dtype != torch.int64 or vert_mesh.dim() != 1 or (nv is not None and vert_mesh.numel() != nv):
        raise RuntimeError("info['vert_mesh'] must be int64 [%s], one id per vertex (got %s %s)"
                           % ("Vt" if nv is None else nv, vert_mesh.dtype, tuple(vert_mesh.shape)))
    return faces, face_list, face_mesh, vert_mesh, int(info["b"])


def ragged_adj_init(faces_union, vert_mesh, b):
    """The info of a ragged batch of b meshes held as one union mesh -- faces_union [Ft,3] int64 into the concatenated vertices,
    vert_mesh int64 [Vt] the mesh of every vertex --, what adj_init + calc_face_list are to one mesh: {'faces', 'face_list'
    (calc_face_list works on a union as it stands), 'face_mesh' int64 [Ft] (ragged.face_mesh: one id per face ever made, dead
    ones included), 'vert_mesh', 'csr' (ragged.csr_from_faces: pass it wherever a layer takes `adj`), 'b'}.  There is no 'adj'
    and no 'adj_orig': a union never forms a dense [Vt,Vt] matrix.  Set-up code: torch ops and their host reads."""
    from . import ragged
    if not torch.is_tensor(faces_union) or faces_union.dim() != 2 or faces_union.shape[1] != 3 or faces_union.dtype != torch.int64:
        raise RuntimeError("faces must be an [Ft,3] int64 tensor (got %s)" % (
            "%s %s" % (faces_union.dtype, tuple(faces_union.shape)) if torch.is_tensor(faces_union) else type(faces_union).__name__))
    if not torch.is_tensor(vert_mesh) or vert_mesh.dim() != 1 or vert_mesh.dtype != torch.int64:
        raise RuntimeError("vert_mesh must be a one-dimensional int64 tensor (got %s)" % (
            "%s %s" % (vert_mesh.dtype, tuple(vert_mesh.shape)) if torch.is_tensor(vert_mesh) else type(vert_mesh).__name__))
    faces = faces_union.contiguous()
    return {"faces": faces, "face_list": calc_face_list(faces), "face_mesh": ragged.face_mesh(faces, vert_mesh).contiguous(),
            "vert_mesh": vert_mesh.contiguous(), "csr": ragged.csr_from_faces(faces, vert_mesh.numel()), "b": int(b)}


_ragged_active_cache = ByTensor()   # (face_list, faces, face_mesh) -> (the active faces, their mesh ids)


def ragged_active_faces(info):
    """(faces[face_list[:, 0, 2]], face_mesh[face_list[:, 0, 2]]): the active faces of a union and the mesh of each -- the pair
    ragged_point_to_surface and ragged_stage_regularisers take.  Cached per TENSOR OBJECTS and in-place versions, as
    active_faces: the tables those functions key on the pair are built once per topology."""
    face_list, faces, face_mesh = info["face_list"], info["faces"], info["face_mesh"]
    hit = _ragged_active_cache.get(face_list, faces, face_mesh)
    if hit is None:
        with torch.no_grad():
            own = face_list[:, 0, 2]
            hit = _ragged_active_cache.put((faces.index_select(0, own).contiguous(), face_mesh.index_select(0, own).contiguous()),
                                           face_list, faces, face_mesh)
    return hit


def ragged_calc_curve(verts, info, angle=70):
    """calc_curve for every mesh of a union at once: (splitting int64 [S], counts int64 [b]).  `splitting` lists mesh 0's
    positions into info['face_list'], then mesh 1's, ...: per mesh what calc_curve selects on that mesh alone -- the rows above
    `angle` ascending, or below three of them the mesh's OWN three most curved faces, largest first, the lower position first
    on ties, NaN never -- because the curvature launch is the same (each face has the bits it has on its mesh alone) and the
    selection walks each mesh's rows separately (a workgroup per mesh, two launches, no atomics: two runs give the same bits).
    counts[m] = how many entries mesh m contributed, on the device.  A row whose mesh id is outside [0, b) is never selected.
    Three launches and ONE host read of two words: S, and the number of meshes with fewer than three faces that have a
    curvature, which raises as calc_curve does.  Not differentiable."""
    from . import ragged
    faces, face_list, face_mesh, _, b = _ragged_info(info)
    curvature = ops.face_curvature(verts, faces, face_list)
    row_list, row_off = ragged.group_rows(face_list, face_mesh, b)
    selected, counts, totals = ops.select_faces_ragged(curvature, angle, row_list, row_off)
    total, short = totals.tolist()                      # the one host read
    if short:
        raise RuntimeError("ragged_calc_curve: %d of the %d meshes have fewer than 3 faces with a curvature (degenerate or too "
                           "small a mesh)" % (short, b))
    return selected[:total], counts


def ragged_split_info(info, verts, features, splitting):
    """split_info on the union of a ragged batch (info: ragged_adj_init or an earlier call's), minus the dense matrices: returns
    (new_info, new_verts [Vt+S,3], new_features [Vt+S,C]).  `splitting`: unique positions into info['face_list'] in [0, Fa), not
    checked (ragged_calc_curve's list); S = splitting.numel().  new_info has the keys of ragged_adj_init: 'faces' [Ft+3S,3] and
    'face_list' [Fa+2S,3,3] by the launch split_info uses (geom_face_split_tables, dense matrices off), 'vert_mesh' [Vt+S] and
    'face_mesh' [Ft+3S] (old ids, then every new vertex and child the mesh of its split face), 'csr' the normalised adjacency
    from the same launch (pass it wherever a layer takes `adj`; ragged_stage_regularisers reads its rowptr / col / inv_deg).
    The vertices are ops.SplitVertices: the union's new rows and both gradients carry the existing kernels' bits.
      * restricted to mesh m and relabelled by rank inside the mesh, the result IS split_info's on mesh m alone;
      * no [n,n] tensor is allocated; the index tables come from launches over chunks of the union;
      * nothing is read on the host and the call can be captured in a graph: the csr is layers.csr_from_parts(rowptr, col, val,
        rowptr, col, val_t, derive=False) -- the six arrays; its derived tables (the width of its neighbour table is a host
        decision) are made when a layer or a regulariser first sees it (layers.adjacency_csr), as for the CSR split_info hands
        over with its dense matrices; a later ragged_split_info takes it as it is."""
    from . import layers
    nv = verts.shape[0]
    faces, face_list, face_mesh, vert_mesh, b = _ragged_info(info, nv)
    if features.dim() != 2 or features.shape[0] != nv:
        raise RuntimeError("features %s must have the %d rows of verts" % (tuple(features.shape), nv))
    splitting = torch.as_tensor(splitting, device=verts.device).to(torch.int64).reshape(-1).contiguous()
    if splitting.numel() > face_list.shape[0]:
        raise RuntimeError("ragged_split_info: splitting holds %d positions for %d active faces" % (splitting.numel(), face_list.shape[0]))
    old = info["csr"]
    if not isinstance(old, layers._Csr) or old.rowptr.numel() != nv + 1:
        raise RuntimeError("info['csr'] must be the union's adjacency over the %d rows of verts (ragged.csr_from_faces)" % nv)
    faces = ops._lib.require(faces, "info['faces']", torch.int64, 2, 3)
    face_list = ops._lib.require(face_list, "info['face_list']", torch.int64, 3, 3)
    face_mesh = ops._lib.require(face_mesh, "info['face_mesh']", torch.int64, 1)
    vert_mesh = ops._lib.require(vert_mesh, "info['vert_mesh']", torch.int64, 1)
    ix, vert_mesh_new, face_mesh_new = ops.split_index_ragged(faces, face_list, splitting, nv, vert_mesh, face_mesh)
    t = ops.split_tables(faces, face_list, ix, old.rowptr, old.col, dense=False)
    new_verts, new_features = ops.SplitVertices.apply(verts, features, ix)
    # the pattern is symmetric: it is its own transpose; the normalised matrix's transpose has the columns' 1 / row length
    csr = layers.csr_from_parts(t["rowptr"], t["col"], t["val"], t["rowptr"], t["col"], t["val_t"], derive=False)
    new_info = {"faces": t["new_faces"], "face_list": t["new_face_list"], "face_mesh": face_mesh_new, "vert_mesh": vert_mesh_new,
                "csr": csr, "b": b}
    return new_info, new_verts, new_features


# ------------------------------------------------------------------- sampling ----
def batch_sample(verts, faces, num=10000, draws=None):
    """Area-weighted random surface points [B,num,3], differentiable in verts
    (reference utils.py:590-633).  `draws=(choices, u, v)` replays pre-drawn randoms
    (choices [B,num] int64 face ids, u already sqrt'ed) -- used by the parity tests."""
    if draws is None:
        draws = ops.draw_samples(verts, faces, num)
    choices, u, v = draws
    return ops.SampleFaces.apply(verts, faces, choices.reshape(verts.shape[0], -1),
                                 u.reshape(verts.shape[0], -1), v.reshape(verts.shape[0], -1))


# --------------------------------------------------------------------- losses ----
def _f_score(sq_to_pred, sq_to_gt, num):
    """F1 at the reference's scale/threshold (utils.py:424-436, 489-500): recall over gt points,
    precision over predicted points, both divided by `num`; averaged over the batch.
    sqrt((.57 d)^2) <= 1e-2 is evaluated from the squared NN distances; one host read."""
    recall = (torch.sqrt(sq_to_pred) * F1_SCALE <= F1_THRESHOLD).sum(1).double() / float(num)
    precision = (torch.sqrt(sq_to_gt) * F1_SCALE <= F1_THRESHOLD).sum(1).double() / float(num)
    f = 2 * (precision * recall) / (precision + recall + 1e-8)
    return float(f.mean())


def _surface_loss(pred_vert, adj_info, gt_points, num, f1, draws, two_sided, loss_out=None, gt_index=None, weight=1.0):
    faces = adj_info["faces"]
    points = tri_ws = None
    if draws is None:   # one kernel draws AND gathers the points (and, for the one-sided loss, prepares the triangle
        #                 records of the scan: both depend only on the vertex positions); replayed draws: separate gather
        if two_sided:
            choices, u, v, points = ops.draw_samples(pred_vert, faces, num, with_points=True)
        else:
            choices, u, v, points, tri_ws = ops.draw_samples(pred_vert, faces, num, with_points=True,
                                                             prepare_scan_for=gt_points.shape[1], gt_index=gt_index)
    else:
        choices, u, v = draws
    mesh_weight = None
    if isinstance(weight, torch.Tensor):      # per-mesh factors: the loss's own scale stays, the kernels apply the factors
        mesh_weight, weight = weight, 1.0
    # the nearest sampled point of every gt point: read by the F1 score, the two-sided loss and the inspection hook only
    need_gt_nn = bool(f1) or two_sided or ops.scan_capture is not None or ops.nn_both_directions
    loss, sq_gt, sq_pred = ops.SurfaceLoss.apply(pred_vert, faces, gt_points, choices, u, v, two_sided, LOSS_SCALE * weight,
                                                 points, tri_ws, loss_out, gt_index, mesh_weight, need_gt_nn)
    if f1:
        return loss, _f_score(sq_gt, sq_pred, num)
    return loss


def batch_point_to_point(pred_vert, adj_info, gt_points, num=1000, f1=False, draws=None, loss_out=None):
    """Two-sided Chamfer loss between sampled surface points and gt (reference utils.py:393-438).
    One fused autograd node (ops.SurfaceLoss); `draws` replays pre-drawn randoms; `loss_out` (one fp32 device element)
    receives the loss -- the returned tensor aliases it (a data-parallel step points it at its all-reduce bucket)."""
    return _surface_loss(pred_vert, adj_info, gt_points, num, f1, draws, True, loss_out)


def batch_point_to_surface(pred_vert, adj_info, gt_points, num=1000, f1=False, draws=None, loss_out=None, gt_index=None,
                           weight=1.0):
    """Chamfer (prediction -> gt) + point-to-surface (gt -> mesh) loss (reference utils.py:441-502); `draws`, `loss_out`
    as for batch_point_to_point.  gt_index (optional, an ops.GtIndex built once for `gt_points`): the Chamfer tiles take
    the culled scan and the draw launch generates the samples in face-visiting order (other, equally distributed draws than
    without the index: sorted uniforms from exponential spacings); on the same draws loss and gradients are those of the plain
    route, bit for bit (tests/test_ops_parity_gpu.py).  weight (not a reference argument): a factor folded into the loss's
    own scale -- `weight * loss` without the multiply launches forward and backward (GEOMetrics.py:138: .2 / .2 / 2); or a
    [B] fp32 tensor of PER-MESH factors: the result is (1/B) sum_m weight[m] * L_m with L_m the loss of mesh m alone -- the
    three stages of the cascade stacked into one call (`torch.cat((p1, p2, p3))` against `torch.cat((gt, gt, gt))`, weights
    3 x (.2, .2, 2) per stage: the mean is over the stacked batch): one draw / scan / finalize / gather launch instead of three."""
    return _surface_loss(pred_vert, adj_info, gt_points, num, f1, draws, False, loss_out, gt_index, weight)


def _ragged_surface_loss(verts, faces, face_mesh, gt_points, num, f1, draws, two_sided, weight=1.0):
    from . import ragged
    if gt_points.dim() != 3:
        raise RuntimeError("gt_points must be [B,N,3] (got shape %s)" % (tuple(gt_points.shape),))
    if face_mesh.dim() != 1 or face_mesh.shape[0] != faces.shape[0]:
        raise RuntimeError("face_mesh must hold one mesh id per face: [%d] (got shape %s)" % (faces.shape[0], tuple(face_mesh.shape)))
    b = gt_points.shape[0]
    mesh_weight = None
    if isinstance(weight, torch.Tensor):      # per-mesh factors: the loss's own scale stays, the kernels apply the factors
        if weight.shape != (b,) or weight.dtype != torch.float32 or weight.device != gt_points.device:
            raise RuntimeError("a per-mesh weight must be a [%d] float32 tensor on %s (got %s %s on %s)"
                               % (b, gt_points.device, weight.dtype, tuple(weight.shape), weight.device))
        mesh_weight, weight = weight, 1.0
    elif isinstance(weight, bool) or not isinstance(weight, (int, float)):
        raise RuntimeError("weight must be a python float or a [B] float32 tensor (got %s)" % type(weight).__name__)
    face_list, face_off = ragged.group_faces(face_mesh, b, faces)
    face_pos = ragged.face_positions(face_mesh, b, faces)
    points = None
    if draws is None:       # one launch draws AND gathers the points
        choices, u, v, points = ops.draw_samples_ragged(verts, faces, face_list, face_off, num, with_points=True)
    else:
        choices, u, v = draws
    need_gt_nn = bool(f1) or two_sided
    loss, sq_gt, sq_pred = ops.RaggedSurfaceLoss.apply(verts, faces, face_list, face_off, gt_points, choices, u, v, two_sided,
                                                       LOSS_SCALE * float(weight), points, need_gt_nn, mesh_weight, face_pos)
    if f1:
        return loss, _f_score(sq_gt, sq_pred, num)
    return loss


def ragged_point_to_surface(verts, faces, face_mesh, gt_points, num=1000, f1=False, draws=None, weight=1.0):
    """batch_point_to_surface for a RAGGED batch: B meshes with their own faces, as after an adaptive split.  verts [Vt,3]
    fp32 (differentiable): the meshes' vertices concatenated, as in ragged.RaggedMeshBatch; faces [Ft,3] int64 into verts: the
    faces the loss runs on (active_faces for split meshes); face_mesh [Ft] in [0, B): the mesh of every face, in any order
    (ragged.face_mesh derives it from per-vertex ids); gt_points [B,N,3].  Value: the mean over m of
    batch_point_to_surface(verts[None], {'faces': the faces of mesh m}, gt_points[m:m+1], num) -- 3000 * (sum sq_pred / (B num)
    + sum sq_tri / (B N)) -- in ONE call: neither search crosses from one mesh into another and every mesh gets `num`
    samples.  draws=(choices [B,num] UNION face ids, u, v) replays draws.  No host read unless f1=True, no padding.  Each
    mesh may hold 1 to 16384 faces; a mesh outside that makes the loss NaN (ops.draw_samples_ragged).  weight, as
    batch_point_to_surface's: a factor folded into the loss's own scale (`weight * loss` without the multiply launches), or a
    [B] fp32 tensor of PER-MESH factors -- the result is (1/B) sum_m weight[m] * L_m with L_m the loss of mesh m alone: the three
    stages of the cascade stacked into one call (their unions concatenated into one union of 3B meshes, whatever their
    topologies, against `torch.cat((gt, gt, gt))`, weights 3 x (.2, .2, 2) per stage: the mean is over the stacked batch).
    The gradient is bit-reproducible: the ordered backward of ops.RaggedSurfaceLoss (GEOM_RAGGED_BACKWARD=scatter: the fp32-atomic
    scatter, float weights only)."""
    return _ragged_surface_loss(verts, faces, face_mesh, gt_points, num, f1, draws, False, weight)


def ragged_point_to_point(verts, faces, face_mesh, gt_points, num=1000, f1=False, draws=None, weight=1.0):
    """batch_point_to_point for a ragged batch: arguments and contract as ragged_point_to_surface, the mean over m of
    batch_point_to_point on mesh m alone."""
    return _ragged_surface_loss(verts, faces, face_mesh, gt_points, num, f1, draws, True, weight)


def calc_point_to_line(p, triangles, point_options):
    """mean |closest(p; a,b,c, option) - p|^2 for per-point triangles (reference utils.py:506-550).
    p [N,3]; triangles = (a, b, c) each [N,3]; point_options [N] int."""
    a, b, c = triangles
    n = p.shape[0]
    verts = torch.cat([a, b, c], dim=0).unsqueeze(0)                       # [1,3N,3]
    ar = torch.arange(n, device=p.device, dtype=torch.int64)
    faces = torch.stack([ar, ar + n, ar + 2 * n], dim=1)                   # triangle i = rows (i, N+i, 2N+i)
    index = ar.to(torch.int32).unsqueeze(0)
    option = point_options.reshape(1, n).to(torch.int32).contiguous()
    total = ops.PointToTriangleSum.apply(p.reshape(1, n, 3), verts, faces, option, index.contiguous())
    return total / n


class edge:
    """Edge a->b with the reference's accessor names (utils.py:553-570)."""

    def __init__(self, a, b):
        self.A = a.clone()
        self.B = b.clone()
        self.Delta = b - a

    def PointAt(self, t):
        return self.A + t.unsqueeze(-1) * self.Delta

    def LengthSquared(self):
        return (self.Delta ** 2).sum(-1)

    def Project(self, p):
        return ((p - self.A) * self.Delta).sum(-1) / self.LengthSquared()


class Plane:
    """Plane through `point` with unit normal `direction/|direction|` (utils.py:573-587)."""

    def __init__(self, point, direction):
        self.Point = point.clone()
        self.Direction = direction / direction.norm(dim=-1, keepdim=True)

    def IsAbove(self, q):
        return (q * self.Point).sum(-1) <= 0

    def Project(self, point):
        h = ((point - self.Point) * self.Direction).sum(-1, keepdim=True)
        return point - h * self.Direction


# ---------------------------------------------------- regularisers ----
def batch_calc_edge(verts, info):
    """Mean squared edge length over the three edges of every face (reference utils.py:636-651):
    one kernel forward, one backward instead of three [B,F,3] gathers and six elementwise passes."""
    faces = info["faces"]
    return ops.EdgeSqLenSum.apply(verts, faces) / (3.0 * verts.shape[0] * faces.shape[0])


def batch_get_lap_info(positions, adj_info):
    """positions - mean(neighbours) (reference utils.py:654-662).  The reference multiplies by the
    dense binary adjacency (26 MB per call at V=2562, six calls per step); here its CSR is built once
    and a thread per vertex walks its row."""
    from .layers import adjacency_csr
    csr = adjacency_csr(adj_info["adj_orig"])
    if positions.dim() == 2:      # the template mesh itself, [V,3] (GEOMetrics.py:156): the reference's matmul broadcasts
        return ops.Laplacian.apply(positions.unsqueeze(0), csr.rowptr, csr.col, csr.inv_deg).squeeze(0)
    return ops.Laplacian.apply(positions, csr.rowptr, csr.col, csr.inv_deg)


def stage_regularisers(prev, cur, adj_info, lap_weight=1.0, move_weight=0.0, edge_weight=0.0):
    """edge_weight * batch_calc_edge(cur) + lap_weight * mean(sum((lap(prev) - lap(cur))^2, 2)) + move_weight *
    mean(sum((prev - cur)^2, 2)) with lap = batch_get_lap_info: the three regularisers the reference's driver adds per
    deformation stage (GEOMetrics.py:147-161), as ONE autograd node with one launch per direction (ops.StageRegularisers) --
    the same value as the driver's expressions built from batch_calc_edge / batch_get_lap_info (tests).  prev: [B,V,3] or
    the [V,3] template.  Not a name of the reference: a driver that wants its regulariser glue off the launch count calls it."""
    from .layers import adjacency_csr
    csr = adjacency_csr(adj_info["adj_orig"])
    return ops.StageRegularisers.apply(prev, cur, adj_info["faces"], csr.rowptr, csr.col, csr.inv_deg, lap_weight, move_weight,
                                       edge_weight)


def ragged_stage_regularisers(prev, cur, faces, face_mesh, vert_mesh, csr, b, lap_weight=1.0, move_weight=0.0, edge_weight=0.0):
    """stage_regularisers for a RAGGED batch: b meshes with their own topology, as after an adaptive split, on ONE union mesh
    (DESIGN.md section 4e).  prev, cur [Vt,3] fp32 (both differentiable): the union's vertices in any order; faces [Ft,3]
    int64 into the union: the faces the edge term runs on (active_faces); face_mesh [Ft], vert_mesh [Vt]: the mesh of every
    face / vertex, in any order -- an id outside [0, b) belongs to no mesh: no term, but its position is still read by its
    neighbours' Laplacians; csr: the union's adjacency (ragged.csr_from_faces, RaggedMeshBatch.csr), None: the edge term
    alone; each weight a python float or a [b] fp32 device tensor (not differentiable).  Value:
        (1/b) sum_m [ w_edge[m] calc_edge(cur_m, faces_m) + w_lap[m] mean_{v in m} |lap(prev)_v - lap(cur)_v|^2
                      + w_move[m] mean_{v in m} |prev_v - cur_v|^2 ]
    -- the mean over m of stage_regularisers on mesh m alone, in ONE autograd node with one launch per direction and no host
    read once the per-mesh counts and the coefficient table are cached (per id / weight tensor OBJECTS).  With [b] weights
    three stages stacked into one union of 3b meshes are one call.  A mesh of [0, b) without a vertex, or without a face at an
    edge weight other than 0, makes the value NaN (the reference's mean over nothing)."""
    from . import ragged
    from .layers import adjacency_csr
    b = int(b)
    if b < 1:
        raise RuntimeError("a ragged batch holds at least one mesh (b = %d)" % b)
    no_edge = not torch.is_tensor(edge_weight) and float(edge_weight) == 0.0
    if csr is None:
        fm, _, coef = ragged.regulariser_tables(face_mesh, None, b, 0.0, 0.0, edge_weight)
        return ops.RaggedStageRegularisers.apply(None, cur, faces, fm, None, coef, None, None, None)
    csr = adjacency_csr(csr)
    if csr.nv != cur.shape[0]:
        raise RuntimeError("the adjacency has %d rows, the union %d vertices" % (csr.nv, cur.shape[0]))
    fm, vm, coef = ragged.regulariser_tables(face_mesh, vert_mesh, b, lap_weight, move_weight, edge_weight)
    return ops.RaggedStageRegularisers.apply(prev, cur, None if no_edge else faces, fm, vm, coef, csr.rowptr, csr.col, csr.inv_deg)


def ragged_calc_edge(verts, faces, face_mesh, b):
    """batch_calc_edge for a ragged batch: the mean over the meshes of calc_edge(verts_m, faces_m) (reference utils.py:636-651)
    on the union's verts [Vt,3]; arguments as ragged_stage_regularisers.  No adjacency is needed or touched."""
    return ragged_stage_regularisers(None, verts, faces, face_mesh, None, None, b, 0.0, 0.0, 1.0)


# ------------------------------------------------ image-feature pooling ----
def batch_camera_info(param):
    """Camera rotation rows [B,3,3] and position [B,3] from (azimuth deg, elevation deg, distance)
    (reference utils.py:286-313).  fp32 parameters on a HIP device that need no gradient: ONE launch
    (geom_camera_info_f32: the same expressions in the same order); anything else: the torch ops below."""
    if (torch.is_tensor(param) and param.is_cuda and param.dtype == torch.float32 and param.dim() == 2 and param.shape[1] >= 3
            and not (param.requires_grad and torch.is_grad_enabled())):
        from . import _lib
        p3 = param[:, :3].contiguous()
        b = p3.shape[0]
        cam_mat = torch.empty(b, 3, 3, dtype=torch.float32, device=param.device)
        cam_pos = torch.empty(b, 3, dtype=torch.float32, device=param.device)
        _lib.call("geom_camera_info_f32", b, p3, cam_mat, cam_pos)
        return cam_mat, cam_pos
    theta = (math.pi * param[:, 0] / 180.0) % 360.0
    phi = (math.pi * param[:, 1] / 180.0) % 360.0
    cam_y = param[:, 2] * torch.sin(phi)
    flat = param[:, 2] * torch.cos(phi)
    cam_pos = torch.stack((flat * torch.cos(theta), cam_y, flat * torch.sin(theta)), dim=1)
    axis_z = cam_pos.clone()
    up = torch.zeros_like(axis_z)            # (0,1,0) built on the device: no host->device copy, graph-capturable
    up[:, 1] = 1.0
    axis_x = torch.cross(up, axis_z, dim=1)
    axis_y = torch.cross(axis_z, axis_x, dim=1)
    rows = [a / torch.sqrt((a ** 2).sum(1)).unsqueeze(-1) for a in (axis_x, axis_y, axis_z)]
    return torch.stack(rows, dim=1), cam_pos


def _is_proj(img_info):
    """Whether img_info is the old driver's projection matrices, a [B,4,4] tensor ([B,3] and longer rows are camera parameters)."""
    return torch.is_tensor(img_info) and img_info.dim() == 3


def _check_proj(proj, b, device, what):
    """The matrix route's argument checks, before any launch: fp32 [b,4,4] on the vertices' device."""
    if proj.dim() != 3 or tuple(proj.shape[1:]) != (4, 4):
        raise RuntimeError("the projection matrices must be a [B,4,4] tensor, one row-major 4 x 4 matrix per %s (got %s)"
                           % (what, str(tuple(proj.shape))))
    if proj.dtype != torch.float32:
        raise RuntimeError("the projection matrices must be fp32 (got %s)" % proj.dtype)
    if proj.shape[0] != b:
        raise RuntimeError("one projection matrix per %s: got %d for %d" % (what, proj.shape[0], b))
    if proj.device != device:
        raise RuntimeError("the projection matrices live on %s, the vertices on %s" % (proj.device, device))
    return proj.detach()


def pooling(blocks, verts_pos, matrix):
    """The old driver's pooling(blocks, verts_pos, matrix) (reference old_GEOMetrics/utils.py:379-427), name and argument order:
    blocks, the fp32 feature maps [C_l, d, d] of ONE image; verts_pos [V,3] fp32; matrix [4,4] fp32, the image's projection matrix
    as the render script wrote it (batch['mats']: projection x model-view).  Returns [V, sum C], differentiable in the maps and
    in the positions; the matrix is data and gets no gradient.  q = matrix . (x, y, z, 1), ys = (q0 / q3 + 1) / 2, xs = 1 -
    (q1 / q3 + 1) / 2 (row 2 of the matrix is never read), then batched_pooling's clamp, weights and texels (DESIGN.md section
    4h).  The batched matrix route at b = 1 on VIEWS of the arguments: no copy of a map, one launch forward, two backward."""
    blocks = list(blocks)
    for blk in blocks:
        if not torch.is_tensor(blk) or blk.dtype != torch.float32 or blk.dim() != 3 or blk.shape[1] != blk.shape[2]:
            raise RuntimeError("feature maps must be fp32 [C, dim, dim] tensors with square planes, the maps of one image (got %s)"
                               % ("%s %s" % (blk.dtype, tuple(blk.shape)) if torch.is_tensor(blk) else type(blk).__name__))
    if not torch.is_tensor(verts_pos) or verts_pos.dtype != torch.float32 or verts_pos.dim() != 2 or verts_pos.shape[1] != 3:
        raise RuntimeError("verts_pos must be an fp32 [V,3] tensor (got %s)"
                           % ("%s %s" % (verts_pos.dtype, tuple(verts_pos.shape)) if torch.is_tensor(verts_pos)
                              else type(verts_pos).__name__))
    if not torch.is_tensor(matrix) or matrix.dim() != 2:
        raise RuntimeError("matrix must be a [4,4] tensor, the image's projection matrix (got %s)"
                           % (str(tuple(matrix.shape)) if torch.is_tensor(matrix) else type(matrix).__name__))
    proj = _check_proj(matrix[None], 1, verts_pos.device, "image")
    if not blocks:
        raise RuntimeError("pooling needs at least one feature map")
    return ops.PoolFeaturesProj.apply(verts_pos[None], proj, 0, *[blk[None] for blk in blocks])[0]


def batched_pooling(blocks, verts_pos, img_info, headroom=0, fronts=None):
    """[B,V,sum C] image features bilinearly pooled from the encoder maps `blocks` (each [B,C,d,d]) at the
    pixels the vertices project to (reference utils.py:316-389).  Differentiable in the maps and in the
    vertex positions; one HIP kernel per direction instead of ~40 eager ops per call.
    headroom (not a reference argument): how many columns the caller is going to concatenate IN FRONT of the result
    (GEOMetrics.py:123,128: the previous features; models.py:241: the 3 coordinates) -- the features are then written as the
    trailing columns of a buffer that wide and `concat_features` / the deformation block fill the front in place of torch.cat.
    fronts (with headroom; not a reference argument): those very tensors, left to right as they will stand in front of the
    features -- e.g. (positions, previous_features) -- which the pooling launch then copies into place itself (the later
    concatenations find them there and copy nothing; gradients flow as before)."""
    # img_info: the camera parameters [B,3], or -- a driver that pools three times per step with the same cameras
    # (GEOMetrics.py:118-128) -- the (cam_mat, cam_pos) pair batch_camera_info(img_info) returned once, or -- the old driver's
    # data (batch['mats']) -- an fp32 [B,4,4] tensor of projection matrices: the matrix route, see pooling()
    room = int(headroom) if not fronts else (int(headroom), tuple(fronts))
    if _is_proj(img_info):
        if not torch.is_tensor(verts_pos) or verts_pos.dim() != 3:
            raise RuntimeError("verts_pos must be a [B,V,3] tensor")
        return ops.PoolFeaturesProj.apply(verts_pos, _check_proj(img_info, verts_pos.shape[0], verts_pos.device, "mesh"), room, *blocks)
    cam_mat, cam_pos = img_info if isinstance(img_info, (tuple, list)) else batch_camera_info(img_info)
    return ops.PoolFeatures.apply(verts_pos, cam_mat.detach(), cam_pos.detach(), room, *blocks)


def ragged_pooling(blocks, verts_union, vert_mesh, img_info):
    """batched_pooling for a RAGGED batch: B meshes with their own vertex counts, as after an adaptive split, on ONE union mesh
    (DESIGN.md section 4f).  blocks: the encoder maps, each [B,C,d,d] fp32; verts_union [Vt,3] fp32: the union's vertices in any
    order (after split_info on a union the new vertices stand at the end: the meshes interleave); vert_mesh [Vt] int32 or int64:
    the mesh of every vertex; img_info: [B,3] camera parameters, batch_camera_info's (cam_mat, cam_pos) or an fp32 [B,4,4] tensor
    of projection matrices (the old driver's batch['mats']: the matrix route, ops.RaggedPoolFeaturesProj), as batched_pooling
    takes it.  Returns [Vt, sum C]: row v is batched_pooling's row for that vertex as a vertex of mesh vert_mesh[v] alone (maps
    blocks[l][m:m+1], camera m), bit for bit.  Differentiable in the maps and in the positions, ONE autograd node
    (ops.RaggedPoolFeatures), one launch forward and two backward, no host read once the grouping of the vertices is cached
    (per vert_mesh tensor OBJECT: ragged.group_vertices).  A vertex whose id is outside [0, B) belongs to no mesh: its row and
    its position gradient are zeros and no map gradient hears of it; a mesh without vertices gets an all-zero map gradient."""
    from . import ragged
    blocks = list(blocks)
    if not blocks:
        raise RuntimeError("ragged_pooling needs at least one feature map")
    for blk in blocks:
        if not torch.is_tensor(blk) or blk.dtype != torch.float32 or blk.dim() != 4 or blk.shape[2] != blk.shape[3]:
            raise RuntimeError("feature maps must be fp32 [B, C, dim, dim] tensors with square planes (got %s)"
                               % ("%s %s" % (blk.dtype, tuple(blk.shape)) if torch.is_tensor(blk) else type(blk).__name__))
    if not torch.is_tensor(verts_union) or verts_union.dtype != torch.float32 or verts_union.dim() != 2 or verts_union.shape[1] != 3:
        raise RuntimeError("verts_union must be an fp32 [Vt,3] tensor, the union's vertices (got %s)"
                           % ("%s %s" % (verts_union.dtype, tuple(verts_union.shape)) if torch.is_tensor(verts_union)
                              else type(verts_union).__name__))
    if not torch.is_tensor(vert_mesh) or vert_mesh.dtype not in (torch.int32, torch.int64) or vert_mesh.dim() != 1:
        raise RuntimeError("vert_mesh must be a one-dimensional int32 or int64 tensor of mesh ids")
    if vert_mesh.shape[0] != verts_union.shape[0]:
        raise RuntimeError("vert_mesh holds %d ids, the union %d vertices" % (vert_mesh.shape[0], verts_union.shape[0]))
    if _is_proj(img_info):
        b = int(img_info.shape[0])
        proj = _check_proj(img_info, b, verts_union.device, "mesh")
        for blk in blocks:
            if blk.shape[0] != b:
                raise RuntimeError("a feature map holds %d images, the matrices are %d" % (blk.shape[0], b))
        ids, _ = ragged.mesh_counts(vert_mesh, b)
        vert_list, vert_off = ragged.group_vertices(vert_mesh, b)
        return ops.RaggedPoolFeaturesProj.apply(verts_union, ids, vert_list, vert_off, proj, *blocks)
    cam_mat, cam_pos = img_info if isinstance(img_info, (tuple, list)) else batch_camera_info(img_info)
    b = int(cam_pos.shape[0])
    if cam_mat.dtype != torch.float32 or cam_pos.dtype != torch.float32:
        raise RuntimeError("the cameras must be fp32 (got %s, %s)" % (cam_mat.dtype, cam_pos.dtype))
    for blk in blocks:
        if blk.shape[0] != b:
            raise RuntimeError("a feature map holds %d images, the cameras %d" % (blk.shape[0], b))
    ids, _ = ragged.mesh_counts(vert_mesh, b)
    vert_list, vert_off = ragged.group_vertices(vert_mesh, b)
    return ops.RaggedPoolFeatures.apply(verts_union, ids, vert_list, vert_off, cam_mat.detach(), cam_pos.detach(), *blocks)


def fan_out(x, n):
    """n handles on the same tensor, one per consumer (not a reference name): results are those of using `x` n times; the n
    gradients are summed by one launch in a fixed order instead of n - 1 accumulation launches."""
    return ops.FanOut.apply(x, int(n)) if n > 1 else (x,)


def sum_losses(*terms):
    """t0 + t1 + ... for scalar loss terms (not a reference name): one launch forward, none backward."""
    return ops.SumScalars.apply(*terms) if len(terms) > 1 else terms[0]


def concat_features(front, pooled):
    """torch.cat((front, pooled), dim=-1) (GEOMetrics.py:123,128) -- without copying `pooled` when it came from
    batched_pooling(..., headroom=...) with room for `front` (and, in the backward pass, without the slicing copies of the
    concatenation's gradient); a plain torch.cat otherwise."""
    return ops.concat_in_front(front, pooled)
