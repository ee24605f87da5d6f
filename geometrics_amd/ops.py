"""Functional + autograd layer over the C ABI for the HBM-bound stages (sampling, losses).

Every function launches on torch's current stream, allocates its outputs with torch and
never synchronises with the host, so a whole training step can be captured in a HIP graph.
"""
import ctypes
import os
import weakref

import torch

from . import _lib
from . import chamfer_distance as _chamfer
from ._identity import ByTensor, MemoryStamp
from .chamfer_distance import chamfer_nn
from .tri_distance import face_order, faces_in_order, morton_order, tri_distance_indexed


def _f32(t, name, ndim, last=None):
    return _lib.require(t, name, torch.float32, ndim, last)


def face_areas(verts, faces):
    """areas[B,F] = 0.5*|(v0-v1) x (v1-v2)|  (reference utils.py:596-602, un-normalised)."""
    verts = _f32(verts.detach(), "verts", 3, 3)
    faces = _lib.require(faces, "faces", torch.int64, 2, 3)
    b, nv, _ = verts.shape
    out = torch.empty(b, faces.shape[0], dtype=torch.float32, device=verts.device)
    _lib.call("geom_face_areas_f32", b, nv, verts, faces.shape[0], faces, out)
    return out


def device_sum(x, scale=1.0):
    """0-dim tensor scale*sum(x) with a fixed reduction tree (bit-reproducible)."""
    x = x.contiguous()
    out = torch.empty((), dtype=torch.float32, device=x.device)
    _lib.call("geom_sum_f32", x.numel(), x, float(scale), out)
    return out


class SampleFaces(torch.autograd.Function):
    """points[B,S,3] from pre-drawn (choices [B,S] int64 face ids, u [B,S] (sqrt'ed), v [B,S]):
    fused gather + barycentric combination (reference utils.py:615-631); backward scatters
    grad_points into grad_verts with the same weights (what autograd does through the three
    index_selects of the reference, in one kernel)."""

    @staticmethod
    def forward(ctx, verts, faces, choices, u, v):
        verts_c = _f32(verts, "verts", 3, 3)
        faces = _lib.require(faces, "faces", torch.int64, 2, 3)
        choices = _lib.require(choices, "choices", torch.int64, 2)
        u = _f32(u, "u", 2)
        v = _f32(v, "v", 2)
        b, nv, _ = verts_c.shape
        num = choices.shape[1]
        if choices.shape[0] != b or u.shape != choices.shape or v.shape != choices.shape:
            raise RuntimeError("choices/u/v must all be [B,num]")
        points = torch.empty(b, num, 3, dtype=torch.float32, device=verts_c.device)
        _lib.call("geom_sample_faces_fwd_f32", b, nv, verts_c, faces.shape[0], faces, num, choices, u, v, points)
        ctx.save_for_backward(faces, choices, u, v)
        ctx.nv = nv
        return points

    @staticmethod
    def backward(ctx, grad_points):
        faces, choices, u, v = ctx.saved_tensors
        grad_points = grad_points.contiguous()
        b, num, _ = grad_points.shape
        grad_verts = torch.zeros(b, ctx.nv, 3, dtype=torch.float32, device=grad_points.device)
        _lib.call("geom_sample_faces_bwd_f32", b, ctx.nv, faces.shape[0], faces, num, choices, u, v, grad_points, grad_verts)
        return grad_verts, None, None, None, None


class GatherSqDistSum(torch.autograd.Function):
    """sum_j |dst[b, idx[b,j]] - src[b,j]|^2 given the squared distances `sq` the NN scan already
    produced for exactly these pairs (reference utils.py:416-417, 462 recompute them from two
    index_selects).  Differentiable in src and dst."""

    @staticmethod
    def forward(ctx, src, dst, idx, sq):
        ctx.save_for_backward(src, dst, idx)
        return device_sum(sq)

    @staticmethod
    def backward(ctx, grad):
        src, dst, idx = ctx.saved_tensors
        src_c, dst_c = src.contiguous(), dst.contiguous()
        b, n, _ = src_c.shape
        m = dst_c.shape[1]
        need_src, need_dst = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_src = torch.empty_like(src_c) if need_src else None
        g_dst = torch.zeros_like(dst_c) if need_dst else None
        grad = grad.contiguous()
        _lib.call("geom_chamfer_grad_f32", b, n, src_c, m, dst_c, idx, grad, 1.0, g_src, 0, g_dst)
        return g_src, g_dst, None, None


class PointToTriangleSum(torch.autograd.Function):
    """sum_j |q_j - p_j|^2 with q_j the closest point selected by option[b,j] on triangle
    index[b,j] (reference calc_point_to_line, utils.py:506-550).  Differentiable in verts."""

    @staticmethod
    def forward(ctx, xyz, verts, faces, option, index):
        xyz_c = _f32(xyz, "xyz", 3, 3)
        verts_c = _f32(verts, "verts", 3, 3)
        b, n, _ = xyz_c.shape
        nv = verts_c.shape[1]
        dev = xyz_c.device
        sq = torch.empty(b, n, dtype=torch.float32, device=dev)
        closest = torch.empty(b, n, 3, dtype=torch.float32, device=dev)
        weights = torch.empty(b, n, 3, dtype=torch.float32, device=dev)
        _lib.call("geom_p2tri_loss_fwd_f32", b, n, xyz_c, nv, verts_c, faces.shape[0], faces, option, index, sq, closest,
                  weights)
        ctx.save_for_backward(xyz_c, faces, index, closest, weights)
        ctx.nv = nv
        return device_sum(sq)

    @staticmethod
    def backward(ctx, grad):
        xyz, faces, index, closest, weights = ctx.saved_tensors
        b, n, _ = xyz.shape
        grad_verts = torch.zeros(b, ctx.nv, 3, dtype=torch.float32, device=xyz.device)
        grad = grad.contiguous()
        _lib.call("geom_p2tri_loss_bwd_f32", b, n, xyz, ctx.nv, faces.shape[0], faces, index, closest, weights, grad, 1.0,
                  grad_verts)
        return None, grad_verts, None, None, None


_vf_cache = ByTensor()   # faces (extra: the vertex count) -> (vf_ptr, vf_item)


def vertex_faces(faces, nv):
    """Static CSR vertex -> incident (face << 2 | corner), ascending per vertex: what the gather backward walks.
    Built once per faces TENSOR OBJECT / in-place version / vertex count (_identity.ByTensor, as the adjacency CSR is)."""
    hit = _vf_cache.get(faces, extra=nv)
    if hit is not None:
        return hit
    with torch.no_grad():
        flat = faces.reshape(-1)
        if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= nv):
            raise RuntimeError("faces refer to vertices outside [0, %d)" % nv)
        order = torch.argsort(flat, stable=True)                      # position p = 3*face + corner
        vf_item = (((order // 3) << 2) | (order % 3)).to(torch.int32).contiguous()
        vf_ptr = torch.zeros(nv + 1, dtype=torch.int64, device=faces.device)
        vf_ptr[1:] = torch.cumsum(torch.bincount(flat, minlength=nv), 0)
        vf_ptr = vf_ptr.to(torch.int32).contiguous()
    return _vf_cache.put((vf_ptr, vf_item), faces, extra=nv)


class GtIndex:
    """What the culled Chamfer scan of the surface step keeps per ground-truth cloud (static data: built once per batch of
    objects, e.g. by the data loader): a spatially coherent visiting order [B,N] int32 and the index written from it by
    geom_nn_cull_index_f32 (run spheres + the cloud in that order).  `order=None`: a 30-bit Morton order made on the
    device.  Any order gives the same results, bit for bit; a bad one only costs speed."""

    def __init__(self, gt_points, order=None):
        gt = _f32(gt_points.detach(), "gt_points", 3, 3)
        b, n, _ = gt.shape
        if order is None:
            order = torch.stack([morton_order(gt[i]) for i in range(b)]) if b else torch.empty(0, n, dtype=torch.int32, device=gt.device)
        order = _lib.require(order, "order", torch.int32, 2)
        if order.shape != (b, n) or order.device != gt.device:
            raise RuntimeError("order must be an int32 [B,N] permutation per cloud on the clouds' device")
        self.order = order
        self.index = torch.empty(max(int(_lib.lib().geom_nn_cull_index_floats(b, n)), 4), dtype=torch.float32, device=gt.device)
        self.shape, self.device = (b, n), gt.device
        # the stamp HOLDS the cloud's memory: while the index lives the allocator cannot hand that address to another cloud (a
        # recycled address at version 0 would pass the check below and be scanned through the OLD cloud's index)
        self.source = MemoryStamp(gt)
        _lib.call("geom_nn_cull_index_f32", b, n, gt, order, self.index)

    def check(self, gt):
        if tuple(gt.shape[:2]) != self.shape or gt.device != self.device or not self.source.matches(gt):
            raise RuntimeError("this GtIndex was built for another ground-truth tensor (or the tensor was modified since)")


class ScanPrep:
    """What the draw launch of a step prepared for the scan of the same step (ops.draw_samples(prepare_scan_for=...)): the
    triangle records and, on the culled route, the index of the sampled points (which were generated in visiting order)."""
    __slots__ = ("tri_ws", "sample_index")

    def __init__(self, tri_ws, sample_index=None):
        self.tri_ws, self.sample_index = tri_ws, sample_index


# The finalize pass of the one-sided surface loss as extra (role) workgroups of the fused scan launch (csrc/tri_distance.hip:
# ScanTail) instead of a launch of its own; same outputs bit for bit.  False: always the separate launch (the A/B switch).
scan_finalize_tail = True
# FAIL-SAFE of the in-launch roles (they wait for tiles of their own launch; a role that waits in vain gives up, the loss is
# NaN and the backward writes NaN gradients for the meshes whose ordering is missing -- csrc/surface_layout.h: status
# words).  Every eager forward that used the roles sends its status words to pinned host memory behind the launch (no
# synchronisation); the NEXT forward looks at the copies that have landed, and the first time one says "gave up" the roles
# are switched off for the rest of the process (the stand-alone finalize launch takes over: 1 % of a step) with a warning.
# A captured step cannot look (no python runs between replays): it stays loud through the NaN loss and gradients, and
# `finalize_roles_gave_up()` lets a training loop ask at the points where it synchronises anyway.
_roles_watch = []          # [(event, pinned int32 [b + 1])] of recent forwards
_roles_gave_up = False


def _watch_roles(order, b, nf, cap):
    global _roles_gave_up, scan_finalize_tail
    if torch.cuda.is_current_stream_capturing():      # (an event query would invalidate the capture)
        return
    done = [w for w in _roles_watch if w[0].query()]
    for w in done:
        _roles_watch.remove(w)
        if int(w[1].abs().sum()) != 0 and not _roles_gave_up:
            _roles_gave_up = True
            scan_finalize_tail = False
            import warnings
            warnings.warn("geometrics_amd: a finalize role of the fused surface scan gave up waiting (status %s); its loss and "
                          "gradients were NaN.  The roles are switched off for the rest of this process (ops.scan_finalize_tail"
                          " = False): the finalize pass runs as its own launch again." % w[1].tolist())
    if order is None or len(_roles_watch) >= 8:
        return
    words = (b + 4) & ~3
    host = torch.empty(b + 1, dtype=torch.int32, pin_memory=True)
    host.copy_(order[order.numel() - words:order.numel() - words + b + 1], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _roles_watch.append((ev, host))


def finalize_roles_gave_up():
    """True once a finalize role of the fused scan launch has given up in this process (checked without synchronising: call
    it behind a point where the step is known to be complete, e.g. after reading the loss)."""
    _watch_roles(None, 0, 0, 0)
    return _roles_gave_up


# Inspection hook (tests, bench.py's parity spot check): a dict that receives the arg-min outputs of the next SurfaceLoss
# forward passes as they sit on the device -- idx_gt (nearest sampled point of every gt point), idx_pred (nearest gt point of
# every sampled point), the draws (choices, u, v) and sampled points it ran on and, one-sided loss, tri_index / tri_option /
# tri_dist of the point-to-triangle scan.  RaggedSurfaceLoss fills it likewise (per-mesh neighbour indices, UNION face ids; one-
# sided loss: tri_index / tri_option and closest / weights / sq of the closest-point pass).  None: off.
scan_capture = None

# The one-sided loss with f1=False reads only the sampled points' nearest gt points: utils.batch_point_to_surface then leaves
# the other direction of the Chamfer scan out (GEOM_FLAG_NN_SAMPLES_ONLY: half the Chamfer tiles of the scan launch).  True
# (tools, A/B timing: GEOM_NN_DIRECTIONS=both): always scan both directions, as before the flag existed -- same loss and gradient.
nn_both_directions = os.environ.get("GEOM_NN_DIRECTIONS", "") == "both"


class SurfaceLoss(torch.autograd.Function):
    """The whole sampled-surface loss of the reference in one autograd node.

      two_sided=False  batch_point_to_surface (utils.py:441-502):
            3000 * ( mean_s |gt[nn(s)] - pred_s|^2  +  mean_g |closest_on_mesh(g) - g|^2 )
      two_sided=True   batch_point_to_point (utils.py:393-438):
            3000 * ( mean_s |gt[nn(s)] - pred_s|^2  +  mean_g |pred[nn(g)] - g|^2 )

    Forward: [tri scan -> closest point] -> sample -> NN (both directions) -> one two-segment sum, one stream.
    Backward: a gather -- the points are binned by face (integer atomics) and every vertex sums the points on its
    incident faces in a fixed order: no float atomics, no zero-fill, bit-reproducible (csrc/surface_gather.hip); the
    gradient of the sampled points is never materialised.  Returns (loss, sq_gt, sq_pred); the squared NN
    distances feed the F1 score and are not differentiable.  need_gt_nn=False (one-sided loss only): the nearest sampled
    point of every gt point, which only the F1 score and the inspection hook read, is not searched; None stands in sq_gt's
    place."""

    @staticmethod
    def forward(ctx, verts, faces, gt, choices, u, v, two_sided, scale, points=None, tri_ws=None, loss_out=None, gt_index=None,
                mesh_weight=None, need_gt_nn=True):
        """mesh_weight (optional, [B] fp32 on the meshes' device): per-mesh factors -- loss = sum_m w[m] * (mesh m's share of the
        loss above), mesh m's gradient times w[m] (geom_surface_finalize_w_f32 / geom_surface_gather_w_f32)."""
        verts_c = _f32(verts.detach(), "verts", 3, 3)
        gt_c = _f32(gt.detach(), "gt_points", 3, 3)
        faces = _lib.require(faces, "faces", torch.int64, 2, 3)
        b, nv, _ = verts_c.shape
        choices = _lib.require(choices.reshape(b, -1), "choices", torch.int64, 2)
        u = _f32(u.reshape(b, -1), "u", 2)
        v = _f32(v.reshape(b, -1), "v", 2)
        num, n_gt, nf, dev = choices.shape[1], gt_c.shape[1], faces.shape[0], verts_c.device
        if gt_c.shape[0] != b:
            raise RuntimeError("gt_points and verts batch sizes differ")
        if mesh_weight is not None:
            mesh_weight = _f32(mesh_weight.detach(), "mesh_weight", 1)
            if mesh_weight.shape[0] != b or mesh_weight.device != verts_c.device:
                raise RuntimeError("mesh_weight must be [B] on the meshes' device")
        L = _lib.lib()
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        have_points = points is not None      # drawn and gathered by one kernel (ops.draw_samples(with_points=True))
        points = _f32(points.detach(), "points", 3, 3) if have_points else torch.empty(b, num, 3, **f32)
        if points.shape != (b, num, 3):
            raise RuntimeError("points must be [B,num,3] for the given draws")
        if loss_out is None:
            out = torch.empty((), **f32)
        else:     # the caller's memory receives the loss (a data-parallel step: the tail of its all-reduce bucket -- no copy launch)
            if not (loss_out.is_cuda and loss_out.device == dev and loss_out.dtype == torch.float32 and loss_out.numel() == 1):
                raise RuntimeError("loss_out must be ONE fp32 element on the mesh batch's device")
            out = loss_out.detach().view(())
        flags = _chamfer.default_flags()
        # the gt points' direction of the Chamfer scan is left out where nothing reads it (the truncation mode keeps both)
        one_dir = not need_gt_nn and not two_sided and not (flags & _lib.FLAG_REF_TAIL_TRUNC)
        sq_pred, idx_g = torch.empty(b, num, **f32), torch.empty(b, num, **i32)
        sq_gt, idx_p = (None, None) if one_dir else (torch.empty(b, n_gt, **f32), torch.empty(b, n_gt, **i32))
        prep = tri_ws if isinstance(tri_ws, ScanPrep) else None
        if prep is not None:
            tri_ws = prep.tri_ws
        cull = None
        if gt_index is not None and prep is not None and prep.sample_index is not None and not two_sided:
            gt_index.check(gt_c)    # the culled Chamfer tiles: both clouds' indices are there
            cull = _lib.args(_lib.SurfaceCull, gt_index.order, gt_index.index, prep.sample_index, None)
        if not two_sided:
            ws_bytes = L.geom_tri_distance_workspace_bytes(b, n_gt, nf)
            ws_ready = tri_ws is not None and have_points      # written by the draw launch (ops.draw_samples(prepare_scan_for=...))
            if ws_ready and (tri_ws.numel() * 4 < ws_bytes or tri_ws.device != dev):
                raise RuntimeError("tri_ws does not belong to this mesh batch / query count")
            ws = tri_ws if ws_ready else torch.empty(max(ws_bytes, 16) // 4, **f32)
            tri_order = face_order(verts_c, faces)      # cached k-d leaf order of the faces: two-level scan
            tri_d, option, index = torch.empty(b, n_gt, **f32), torch.empty(b, n_gt, **i32), torch.empty(b, n_gt, **i32)
            sq, closest, weights = torch.empty(b, n_gt, **f32), torch.empty(b, n_gt, 3, **f32), torch.empty(b, n_gt, 3, **f32)
        if not have_points:
            _lib.call("geom_sample_faces_fwd_f32", b, nv, verts_c, nf, faces, num, choices, u, v, points)
        # Both arg-min scans -- Chamfer NN in both directions and (one-sided loss) the point-to-triangle scan with
        # the closest point / weights / squared distance of the winner -- in ONE call: one heterogeneous launch
        # behind the triangle-record prep.  (Round 1 ran them back to back: two streams inside a captured graph cost
        # 5-10 us per fork/join edge.)  When a gradient is wanted the scans also write every point's gradient record
        # into the backward scratch.
        want = bool(ctx.needs_input_grad[0])
        order = torch.empty(L.geom_surface_order_words(b, nf, num, n_gt), dtype=torch.int32, device=dev)
        coef_s, coef_o = scale / (b * num), scale / (b * n_gt)
        wrote = ctypes.c_int(0)
        if not two_sided and ws_ready:
            flags |= _lib.FLAG_TRI_WS_READY
        if one_dir:
            flags |= _lib.FLAG_NN_SAMPLES_ONLY
        if two_sided:
            tri_args = (nv, None, nf, None, None, None, None, None, None, None, None)    # nf still sizes the scratch layout
            ws, ws_bytes = None, 0
        else:
            tri_args = (nv, verts_c, nf, faces, tri_order, tri_d, option, index, sq, closest, weights)
        # one-sided loss: the finalize pass (below) rides in the scan launch as extra (role) workgroups where the launch is
        # the fused one and a mesh's faces + points fit its LDS (tail.finalized says so): each mesh is ordered as soon
        # as ITS triangle tiles are through instead of in a launch of its own behind the slowest tile
        tail = None
        if not two_sided and scan_finalize_tail and mesh_weight is None:    # (the in-launch roles know no per-mesh factors)
            tail = _lib.args(_lib.SurfaceTail, choices, scale / sq_pred.numel(), scale / sq.numel(), int(want), out, 0)
        _lib.call("geom_surface_scan_f32", b, n_gt, gt_c, num, points, sq_gt, idx_p, sq_pred, idx_g, *tri_args, u, v, coef_s, coef_o,
                  order if want else None, flags, ws, ws_bytes, ctypes.byref(wrote), cull, tail)
        # finalize: the loss reduction AND, when a gradient is wanted, the backward's preparation (points counting-sorted
        # by face in ascending id order; the records too when the scans could not write them) in one launch; the
        # backward is then a single gather launch
        other_sq = sq_gt if two_sided else sq
        args = (b, nf, num, choices, u, v, points, n_gt, gt_c, idx_g, idx_p if two_sided else None, None if two_sided else index,
                None if two_sided else closest, None if two_sided else weights, sq_pred, other_sq, scale / sq_pred.numel(),
                scale / other_sq.numel(), coef_s, coef_o)
        if tail is None or not tail.finalized:
            code = _lib.status("geom_surface_finalize_w_f32", *args, int(want), wrote.value, order, out, mesh_weight)
            if code == _lib.EUNSUPPORTED:       # too many faces + points for the in-LDS ordering: loss only, scatter backward
                if mesh_weight is not None and want:
                    raise RuntimeError("per-mesh weights need the ordered backward (faces + points of a mesh within ~38 000)")
                want = False
                code = _lib.status("geom_surface_finalize_w_f32", *args, 0, 0, order, out, mesh_weight)
            _lib.check(code, "geom_surface_finalize_w_f32")
        ctx.order = order if want else None
        if tail is not None and tail.finalized and want:
            with torch.cuda.device(dev):      # (the watch records an event and asks about capture on the current stream)
                _watch_roles(order, b, nf, num + n_gt)
        if scan_capture is not None:
            scan_capture.update(idx_gt=idx_p, idx_pred=idx_g, sq_gt=sq_gt, sq_pred=sq_pred, choices=choices, u=u, v=v, points=points)
            if not two_sided:
                scan_capture.update(tri_index=index, tri_option=option, tri_dist=tri_d)
        if two_sided:
            ctx.save_for_backward(faces, choices, u, v, points, gt_c, idx_g, idx_p)
        else:
            ctx.save_for_backward(faces, choices, u, v, points, gt_c, idx_g, index, closest, weights)
        ctx.two_sided, ctx.scale, ctx.nv = two_sided, scale, nv
        ctx.mesh_weight = mesh_weight
        ctx.mark_non_differentiable(*(t for t in (sq_gt, sq_pred) if t is not None))
        ctx.set_materialize_grads(False)    # no zero tensors (two fill launches) for the two distance outputs
        return out, sq_gt, sq_pred

    @staticmethod
    def backward(ctx, grad, _g1, _g2):
        saved = ctx.saved_tensors
        faces, choices, u, v, points, gt = saved[:6]
        b, num, _ = points.shape
        n_gt, nf, nv = gt.shape[1], faces.shape[0], ctx.nv
        dev = points.device
        grad = grad.contiguous()
        if ctx.order is not None:           # prepared by the forward's finalize launch: one gather, no atomics
            vf_ptr, vf_item = vertex_faces(faces, nv)
            grad_verts = torch.empty(b, nv, 3, dtype=torch.float32, device=dev)
            _lib.call("geom_surface_gather_w_f32", b, nv, nf, vf_ptr, vf_item, num, n_gt, 1, ctx.order, grad,
                      ctx.mesh_weight, grad_verts)
        elif ctx.mesh_weight is not None:
            raise RuntimeError("per-mesh weights need the ordered backward")
        else:
            # a mesh whose faces + points do not fit the ordering pass's LDS (> ~38 000 together): scatter formulation
            # (fp32 atomics into a zeroed gradient; same values up to summation order)
            grad_verts = torch.zeros(b, nv, 3, dtype=torch.float32, device=dev)
            if ctx.two_sided:
                for other_idx, via_nn, coef in ((saved[6], 0, ctx.scale / (b * num)), (saved[7], 1, ctx.scale / (b * n_gt))):
                    _lib.call("geom_sample_chamfer_bwd_f32", b, nv, nf, faces, num, choices, u, v, points, n_gt, gt,
                              other_idx, via_nn, grad, coef, grad_verts)
            else:
                index, closest, weights = saved[7:10]
                _lib.call("geom_surface_loss_bwd_f32", b, nv, nf, faces, num, choices, u, v, points, n_gt, gt, saved[6],
                          index, closest, weights, grad, ctx.scale / (b * num), ctx.scale / (b * n_gt), grad_verts)
        return grad_verts, None, None, None, None, None, None, None, None, None, None, None, None, None


class Laplacian(torch.autograd.Function):
    """lap = p - mean(neighbours(p)) over the CSR of the binary adjacency (reference
    batch_get_lap_info, utils.py:654-662, a dense [V,V] @ [B,V,3] there)."""

    @staticmethod
    def forward(ctx, positions, rowptr, col, inv_deg):
        x = _f32(positions, "positions", 3, 3)
        b, nv, _ = x.shape
        out = torch.empty_like(x)
        _lib.call("geom_laplacian_f32", b, nv, rowptr, col, inv_deg, x, 0, out)
        ctx.save_for_backward(rowptr, col, inv_deg)
        return out

    @staticmethod
    def backward(ctx, grad):
        rowptr, col, inv_deg = ctx.saved_tensors
        g = grad.contiguous()
        b, nv, _ = g.shape
        out = torch.empty_like(g)
        _lib.call("geom_laplacian_f32", b, nv, rowptr, col, inv_deg, g, 1, out)
        return out, None, None, None


class EdgeSqLenSum(torch.autograd.Function):
    """sum over meshes and faces of the three squared edge lengths (reference batch_calc_edge,
    utils.py:636-651, before its means)."""

    @staticmethod
    def forward(ctx, verts, faces):
        v = _f32(verts, "verts", 3, 3)
        faces = _lib.require(faces, "faces", torch.int64, 2, 3)
        b, nv, _ = v.shape
        per_face = torch.empty(b, faces.shape[0], dtype=torch.float32, device=v.device)
        _lib.call("geom_edge_sqlen_fwd_f32", b, nv, v, faces.shape[0], faces, per_face)
        ctx.save_for_backward(v, faces)
        return device_sum(per_face)

    @staticmethod
    def backward(ctx, grad):
        v, faces = ctx.saved_tensors
        b, nv, _ = v.shape
        grad = grad.contiguous()
        grad_verts = torch.zeros_like(v)
        _lib.call("geom_edge_sqlen_bwd_f32", b, nv, v, faces.shape[0], faces, grad, 1.0, grad_verts)
        return grad_verts, None


class FanOut(torch.autograd.Function):
    """n tensor objects over x's memory, one per consumer: their gradients meet in ONE launch (geom_sum_tensors_f32, fixed
    order) instead of autograd's n - 1 accumulation launches.  A stage's positions have six consumers in the reference's
    driver (GEOMetrics.py:118-161)."""

    @staticmethod
    def forward(ctx, x, n):
        from .layers import _alias
        xc = x if x.is_contiguous() else x.contiguous()
        ctx.n = n
        return tuple(_alias(xc) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        def rows(g):      # a [.., width] column slice of a wider row-major buffer is read in place
            if g.is_contiguous():
                return g, g.shape[-1]
            if g.dim() >= 2 and g.stride(-1) == 1 and g.stride(-2) >= g.shape[-1] and \
                    all(g.stride(d) == g.stride(d + 1) * g.shape[d + 1] for d in range(g.dim() - 2)):
                return g, g.stride(-2)
            return g.contiguous(), g.shape[-1]
        given = [rows(g) for g in grads if g is not None]
        if not given:
            return None, None
        first = given[0][0]
        fast = first.is_cuda and first.dtype == torch.float32 and len(given) <= _lib.SUM_MAX_TENSORS and first.dim() >= 1
        if len(given) == 1 or not fast:
            total = first.contiguous()
            for g, _ in given[1:]:
                total = total + g
            return total, None
        out = torch.empty(first.shape, dtype=torch.float32, device=first.device)
        ptrs = [g for g, _ in given]
        width = first.shape[-1]
        if all(ld == width for _, ld in given):
            _lib.call("geom_sum_tensors_f32", len(given), ptrs, out.numel(), out)
        else:
            lds = (ctypes.c_int64 * len(given))(*[ld for _, ld in given])
            _lib.call("geom_sum_tensors_rows_f32", len(given), ptrs, lds, out.numel() // width, width, out)
        return out, None


class SumScalars(torch.autograd.Function):
    """((t0 + t1) + t2) + ... of up to 8 zero-dimensional fp32 tensors in ONE launch (geom_sum_tensors_f32); backward: every term
    receives the incoming gradient itself (no launch).  The driver's `loss = edge_loss + surface_loss + lap_loss + ...`
    (GEOMetrics.py:164) costs a launch per `+` forward and one per term backward."""

    @staticmethod
    def forward(ctx, *terms):
        ts = [t.reshape(()) for t in terms]
        out = torch.empty((), dtype=torch.float32, device=ts[0].device)
        ctx.n = len(ts)
        if not all(t.is_cuda and t.dtype == torch.float32 for t in ts) or len(ts) > _lib.SUM_MAX_TENSORS:
            total = ts[0]
            for t in ts[1:]:
                total = total + t
            return total
        _lib.call("geom_sum_tensors_f32", len(ts), ts, 1, out)
        return out

    @staticmethod
    def backward(ctx, grad):
        return (grad,) * ctx.n


class StageRegularisers(torch.autograd.Function):
    """The regularisers of ONE deformation stage as one scalar (GEOMetrics.py:147-161 on utils.py:636-662):
        w_edge * mean over (mesh, face) of (|e1|^2 + |e2|^2 + |e3|^2)(cur) / 3
      + w_lap  * mean over (mesh, vertex) of |lap(prev) - lap(cur)|^2      + w_move * mean over (mesh, vertex) of |prev - cur|^2
    ONE launch forward (+ the fixed-order sum of its partials), ONE backward (csrc/regularizers.hip) instead of ~45 eager
    launches; prev [B,V,3] or the [V,3] template."""

    @staticmethod
    def forward(ctx, prev, cur, faces, rowptr, col, inv_deg, w_lap, w_move, w_edge):
        c = _f32(cur, "cur", 3, 3)
        b, nv, _ = c.shape
        batched = prev.dim() == 3
        p = _f32(prev, "prev", 3 if batched else 2, 3)
        if batched and p.shape != c.shape or not batched and p.shape[0] != nv:
            raise RuntimeError("prev must be [B,V,3] like cur or one [V,3] mesh")
        faces = _lib.require(faces, "faces", torch.int64, 2, 3)
        nf = faces.shape[0]
        c_lap, c_move = float(w_lap) / (b * nv), float(w_move) / (b * nv)
        c_edge = float(w_edge) / (3.0 * b * nf) if nf else 0.0
        lapd = torch.empty_like(c)
        partial = torch.empty(int(_lib.lib().geom_stage_regularisers_blocks(b, nv, nf)), dtype=torch.float32, device=c.device)
        _lib.call("geom_stage_regularisers_fwd_f32", b, nv, p, int(batched), c, nf, faces, rowptr, col, inv_deg, c_lap, c_move,
                  c_edge, lapd, partial)
        ctx.save_for_backward(p, c, faces, rowptr, col, inv_deg, lapd)
        ctx.coef, ctx.batched = (c_lap, c_move, c_edge), batched
        return device_sum(partial)

    @staticmethod
    def backward(ctx, grad):
        p, c, faces, rowptr, col, inv_deg, lapd = ctx.saved_tensors
        b, nv, _ = c.shape
        c_lap, c_move, c_edge = ctx.coef
        g = grad.contiguous()
        vf_ptr, vf_item = vertex_faces(faces, nv) if c_edge != 0.0 else (None, None)
        want_prev = ctx.needs_input_grad[0]
        grad_cur = torch.empty_like(c)
        grad_prev = torch.empty_like(c) if want_prev else None
        _lib.call("geom_stage_regularisers_bwd_f32", b, nv, p, int(ctx.batched), c, faces.shape[0], faces, rowptr, col, inv_deg,
                  vf_ptr, vf_item, c_lap, c_move, c_edge, lapd, g, grad_prev if ctx.batched else None, grad_cur)
        if want_prev and not ctx.batched:      # a template that asks for its gradient: the sum over the batch of -grad_cur's lap/move part
            raise RuntimeError("StageRegularisers: the gradient with respect to an unbatched [V,3] prev is not implemented")
        return grad_prev, (grad_cur if ctx.needs_input_grad[1] else None), None, None, None, None, None, None, None


class RaggedStageRegularisers(torch.autograd.Function):
    """StageRegularisers for a RAGGED batch on one union mesh: prev, cur [Vt,3]; faces [Ft,3] int64 into
    the union or None (no edge term); face_mesh [Ft], vert_mesh [Vt] int32 mesh ids; coef [3,b] fp32 on the device
    (ragged.regulariser_tables: the weights over each mesh's own counts); (rowptr, col, inv_deg) the union's adjacency, or
    all None: the edge term alone (prev and vert_mesh None as well).  The sum over the vertices and faces of each one's term
    times ITS mesh's coefficient: ONE launch forward (+ the fixed-order sum of its partials), ONE backward, no host read."""

    @staticmethod
    def forward(ctx, prev, cur, faces, face_mesh, vert_mesh, coef, rowptr, col, inv_deg):
        c = _f32(cur, "cur", 2, 3)
        nv = c.shape[0]
        coef = _f32(coef, "coef", 2)
        b = coef.shape[1]
        if coef.shape[0] != 3 or b == 0 or nv == 0:
            raise RuntimeError("coef must be [3,b] with b >= 1 and the union must hold a vertex (got %s, %d vertices)"
                               % (tuple(coef.shape), nv))
        lap = rowptr is not None
        p = lapd = None
        if lap:
            p = _f32(prev, "prev", 2, 3)
            if p.shape != c.shape or vert_mesh.shape != (nv,) or rowptr.numel() != nv + 1 or inv_deg.numel() != nv:
                raise RuntimeError("prev, vert_mesh and the adjacency must describe cur's %d vertices" % nv)
            lapd = torch.empty_like(c)
        nf = 0
        if faces is not None and faces.shape[0]:
            faces = _lib.require(faces, "faces", torch.int64, 2, 3)
            nf = faces.shape[0]
            if face_mesh.shape != (nf,):
                raise RuntimeError("face_mesh must be [%d], one id per face (got %s)" % (nf, tuple(face_mesh.shape)))
        else:
            faces = None
        partial = torch.empty(int(_lib.lib().geom_ragged_regularisers_blocks(nv, nf)), dtype=torch.float32, device=c.device)
        nnz = col.numel() if lap else 0
        _lib.call("geom_ragged_regularisers_fwd_f32", b, nv, p, c, nf, faces, vert_mesh, face_mesh, coef, nnz, rowptr, col, inv_deg,
                  lapd, partial)
        ctx.save_for_backward(p, c, faces, face_mesh, vert_mesh, coef, rowptr, col, inv_deg, lapd)
        return device_sum(partial)

    @staticmethod
    def backward(ctx, grad):
        p, c, faces, face_mesh, vert_mesh, coef, rowptr, col, inv_deg, lapd = ctx.saved_tensors
        nv, b = c.shape[0], coef.shape[1]
        nf = faces.shape[0] if faces is not None else 0
        vf_ptr, vf_item = vertex_faces(faces, nv) if nf else (None, None)
        want_prev = p is not None and ctx.needs_input_grad[0]
        grad_cur = torch.empty_like(c)
        grad_prev = torch.empty_like(c) if want_prev else None
        _lib.call("geom_ragged_regularisers_bwd_f32", b, nv, p, c, nf, faces, vert_mesh, face_mesh, coef,
                  col.numel() if col is not None else 0, rowptr, col, inv_deg, vf_ptr, vf_item, lapd, grad.contiguous(), grad_prev,
                  grad_cur)
        return grad_prev, (grad_cur if ctx.needs_input_grad[1] else None), None, None, None, None, None, None, None


# ---- feature buffers with HEADROOM: concatenation without torch.cat ------------------------------------------------------------
# The driver builds a deformation block's input as cat(positions, cat(previous features, pooled features)) (GEOMetrics.py:118-131,
# models.py:241): two copies of ~35 MB forward per stage, and slicing copies of the same size when the gradient of the
# concatenation is taken apart again.  A pooling call that is told how many columns will be put IN FRONT of its output
# (`headroom`) allocates the wide buffer itself and writes its features at that column offset (geom_pool_features_fwd_fronts_f32); the
# later "concatenations" (`concat_in_front`) only copy the narrow operand into the free columns and widen the view, and in the
# backward pass every consumer reads its column slice of the ONE wide gradient in place.
_headroom = {}     # storage address of a wide buffer -> its _WideBuffer


class _WideBuffer:
    """What the registry knows of one wide buffer: `ref`, a weak reference to it (the entry goes when the buffer does); `free`,
    the columns still free in front of the view handed out; `placed`, {first column: (stamp, width) of a tensor the pooling launch
    already copied there} -- the stamps hold those tensors' memory until the wide buffer dies (_identity.MemoryStamp)."""
    __slots__ = ("ref", "free", "placed")

    def __init__(self, ref, free, placed):
        self.ref, self.free, self.placed = ref, free, placed

    @property
    def buf(self):
        return self.ref()

    def place(self, col, t):
        """Note that columns [col, col + width) are going to hold `t` as it is now."""
        self.placed[col] = (MemoryStamp(t), t.shape[2])

    def holds(self, col, t):
        """Whether columns [col, col + width) already hold `t` (PoolFeatures(fronts=...) copied it there)."""
        hit = self.placed.get(col)
        return hit is not None and hit[1] == t.shape[2] and hit[0].matches(t)


def _register_headroom(buf, free):
    """Enter the wide buffer `buf` with `free` columns in front of the view handed out, or shrink its free columns (what has been
    placed in it stays known).  Returns its record."""
    key = buf.untyped_storage().data_ptr()
    old = _headroom.get(key)
    placed = old.placed if old is not None and old.buf is buf else {}      # (a recycled address: another buffer's record)
    rec = _headroom[key] = _WideBuffer(weakref.ref(buf, lambda _r, k=key: _headroom.pop(k, None)), free, placed)
    return rec


def wide_buffer_of(view):
    """The record of the wide buffer whose storage `view` lives in, or None."""
    rec = _headroom.get(view.untyped_storage().data_ptr())
    return rec if rec is not None and rec.buf is not None else None


def headroom_of(t):
    """Free columns in front of `t` [B,V,C] inside a wide buffer made by PoolFeatures(headroom=...) / concat_in_front, or 0."""
    if not (torch.is_tensor(t) and t.dim() == 3 and t.is_cuda and t.stride(2) == 1):
        return 0
    rec = wide_buffer_of(t)
    if rec is None:
        return 0
    buf, free = rec.buf, rec.free
    ld = buf.shape[2]
    if t.stride(1) != ld or t.stride(0) != t.shape[1] * ld or t.shape[:2] != buf.shape[:2] or t.storage_offset() != free:
        return 0
    return free if free + t.shape[2] == ld else 0


class _ConcatInFront(torch.autograd.Function):
    """cat((front, wide_view), -1) where wide_view has headroom: `front` is copied into the free columns right in front of the
    view and the view grows to cover them -- no copy of the wide operand; backward: the two column slices of the gradient,
    as views."""

    @staticmethod
    def forward(ctx, front, view):
        rec = wide_buffer_of(view)
        buf, free = rec.buf, rec.free
        cf = front.shape[2]
        if not rec.holds(free - cf, front):
            buf[..., free - cf:free].copy_(front)
        out = buf[..., free - cf:]
        _register_headroom(buf, free - cf)
        ctx.cf = cf
        return out

    @staticmethod
    def backward(ctx, g):
        return g[..., :ctx.cf], g[..., ctx.cf:]


def concat_in_front(front, view):
    """torch.cat((front, view), dim=-1) for [B,V,*] tensors -- without touching `view` when it was allocated with headroom for
    `front` (PoolFeatures(headroom=...)); a plain torch.cat otherwise."""
    if (torch.is_tensor(front) and front.dim() == 3 and front.is_cuda and front.dtype == torch.float32 and view.dtype == torch.float32
            and front.shape[:2] == view.shape[:2] and 0 < front.shape[2] <= headroom_of(view)):
        return _ConcatInFront.apply(front, view)
    return torch.cat((front, view), dim=-1)


def _pool_forward_operands(v, headroom, blocks):
    """What the two batched pooling nodes (PoolFeatures, PoolFeaturesProj) hand their forward launch besides the camera, for checked
    vertices v [B,V,3]: (maps, channels, dims, their number, out, out_ld, (n_fronts, fronts, widths, cols, buf)).  headroom: an int or
    (headroom, fronts), see PoolFeatures.forward."""
    fronts = ()
    if isinstance(headroom, (tuple, list)):
        headroom, fronts = headroom
    headroom = int(headroom or 0)
    blks = [_f32(b, "block", 4) for b in blocks]
    b, nv, _ = v.shape
    for blk in blks:
        if blk.shape[0] != b or blk.shape[2] != blk.shape[3]:
            raise RuntimeError("feature maps must be [B, C, dim, dim] with the vertex batch size")
    n = len(blks)
    chans = (ctypes.c_int * n)(*[t.shape[1] for t in blks])
    dims = (ctypes.c_int * n)(*[t.shape[2] for t in blks])
    ctot = sum(t.shape[1] for t in blks)
    srcs, own = [], []       # (contiguous front, its first column); (column, front) of those that are the caller's own tensor
    if fronts:
        col = 0
        for t in fronts:
            if not (torch.is_tensor(t) and t.dim() == 3 and tuple(t.shape[:2]) == (b, nv) and t.is_cuda and t.device == v.device
                    and t.dtype == torch.float32):
                raise RuntimeError("fronts must be fp32 [B,V,*] tensors on the meshes' device")
            c = t.detach().contiguous()
            srcs.append((c, col))
            if c.data_ptr() == t.data_ptr():       # (a copy made here is not what the caller will hand to the concatenation)
                own.append((col, t))
            col += t.shape[2]
        if col != headroom or len(srcs) > 2:
            raise RuntimeError("at most two fronts, whose widths add up to the headroom")
    if headroom > 0:      # the features as the trailing columns of a wider buffer: see concat_in_front
        buf = torch.empty(b, nv, headroom + ctot, dtype=torch.float32, device=v.device)
        out = buf[..., headroom:]
        rec = _register_headroom(buf, headroom)
        for col, t in own:
            rec.place(col, t)
    else:
        buf, out = None, torch.empty(b, nv, ctot, dtype=torch.float32, device=v.device)
    m = len(srcs)
    front_args = (m, [t for t, _ in srcs], (ctypes.c_int * m)(*[t.shape[2] for t, _ in srcs]), (ctypes.c_int * m)(*[c for _, c in srcs]), buf)
    return blks, chans, dims, n, out, headroom + ctot if headroom > 0 else 0, front_args


def _pitched_gradient(grad_out, rows_uniform):
    """(g, pitch): grad_out [..., V, C] in place when it is a column slice of a wider row-major buffer (the block's input gradient;
    rows_uniform: every vertex row, across the leading dimension too, lies one pitch after the last), else a contiguous copy."""
    ctot = grad_out.shape[-1]
    if grad_out.stride(-1) == 1 and grad_out.stride(-2) >= ctot and rows_uniform and grad_out.is_cuda and grad_out.dtype == torch.float32:
        return grad_out, grad_out.stride(-2)
    return grad_out.contiguous(), ctot


class PoolFeatures(torch.autograd.Function):
    """Bilinear pooling of the image feature maps at the projected vertex positions (reference
    batched_pooling, utils.py:316-389): one kernel forward, one backward (texel scatters + closed-form
    chain to the vertex positions)."""

    @staticmethod
    def forward(ctx, verts, cam_mat, cam_pos, headroom, *blocks):
        """headroom: columns left free IN FRONT of the pooled features (0: a plain contiguous result; see concat_in_front), or
        (headroom, fronts): also up to two [B,V,*] tensors, left to right as they will stand in front of the features (their
        widths add up to the headroom), which the launch copies there -- concat_in_front / the deformation block then find them
        in place (the gradient still flows through those nodes: the tensors are not inputs of this one)."""
        v = _f32(verts, "verts_pos", 3, 3)
        cam_mat = _f32(cam_mat, "cam_mat", 3, 3)
        cam_pos = _f32(cam_pos, "cam_pos", 2, 3)
        blks, chans, dims, n, out, out_ld, front_args = _pool_forward_operands(v, headroom, blocks)
        b, nv, _ = v.shape
        _lib.call("geom_pool_features_fwd_fronts_f32", b, nv, v, cam_mat, cam_pos, n, blks, chans, dims, out, out_ld, *front_args)
        ctx.save_for_backward(v, cam_mat, cam_pos, *blks)
        ctx.meta = (chans, dims, n)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        v, cam_mat, cam_pos = ctx.saved_tensors[:3]
        blks = ctx.saved_tensors[3:]
        chans, dims, n = ctx.meta
        b, nv, _ = v.shape
        ctot = grad_out.shape[2]
        # the gradient in place when it is a column slice of a wider row-major buffer (the block's input gradient), else contiguous
        if grad_out.stride(2) == 1 and grad_out.stride(1) >= ctot and grad_out.stride(0) == nv * grad_out.stride(1) and grad_out.is_cuda \
                and grad_out.dtype == torch.float32:
            g, g_ld = grad_out, grad_out.stride(1)
        else:
            g, g_ld = grad_out.contiguous(), ctot
        need_blocks = [ctx.needs_input_grad[4 + i] for i in range(n)]
        gblks = [torch.empty_like(t) if need else None for t, need in zip(blks, need_blocks)]
        gverts = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        ws, ws_bytes = None, 0
        if any(need_blocks) or gverts is not None:
            # texel -> (vertex, weight) lists for the gather formulation of the map gradient + the per-chunk partial sums
            # of the vertex gradient
            ws_bytes = _lib.lib().geom_pool_features_bwd_workspace_bytes(b, nv, n, dims)
            ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=v.device)
        _lib.call("geom_pool_features_bwd_ld_f32", b, nv, v, cam_mat, cam_pos, n, blks, chans, dims, g,
                  g_ld if g_ld != ctot else 0, gblks, gverts, ws, ws_bytes)
        return (gverts, None, None, None) + tuple(gblks)


class RaggedPoolFeatures(torch.autograd.Function):
    """PoolFeatures for a RAGGED batch on one union mesh: verts [Vt,3], the union's vertices in any order;
    vert_mesh [Vt] int32, the mesh of every vertex (ragged.mesh_counts' clamped ids); (vert_list, vert_off) from
    ragged.group_vertices; cam_mat [B,3,3], cam_pos [B,3]; blocks [B,C,d,d].  Row v of the [Vt, sum C] result is PoolFeatures' row
    for vertex v as a vertex of mesh vert_mesh[v] alone; a vertex of no mesh gets zeros and no gradient.  The batched kernels'
    bodies with the mesh per lane: one launch forward, two backward, no host read."""

    @staticmethod
    def forward(ctx, verts, vert_mesh, vert_list, vert_off, cam_mat, cam_pos, *blocks):
        v = _f32(verts, "verts_union", 2, 3)
        cam_mat = _f32(cam_mat, "cam_mat", 3, 3)
        cam_pos = _f32(cam_pos, "cam_pos", 2, 3)
        vert_mesh = _lib.require(vert_mesh, "vert_mesh", torch.int32, 1)
        vert_list = _lib.require(vert_list, "vert_list", torch.int32, 1)
        vert_off = _lib.require(vert_off, "vert_off", torch.int32, 1)
        blks = [_f32(b, "block", 4) for b in blocks]
        vt, b = v.shape[0], cam_pos.shape[0]
        if vt == 0 or b == 0 or not blks:
            raise RuntimeError("the union must hold a vertex, the batch a mesh and a feature map (got %d vertices, %d meshes, %d maps)"
                               % (vt, b, len(blks)))
        if vert_mesh.shape[0] != vt or vert_list.shape[0] != vt or vert_off.shape[0] != b + 1 or cam_mat.shape[0] != b:
            raise RuntimeError("vert_mesh and vert_list must hold one entry per vertex of the union (%d), vert_off and the cameras one "
                               "per mesh (%d)" % (vt, b))
        for blk in blks:
            if blk.shape[0] != b or blk.shape[2] != blk.shape[3]:
                raise RuntimeError("feature maps must be [B, C, dim, dim] with the cameras' batch size")
        n = len(blks)
        chans = (ctypes.c_int * n)(*[t.shape[1] for t in blks])
        dims = (ctypes.c_int * n)(*[t.shape[2] for t in blks])
        out = torch.empty(vt, sum(t.shape[1] for t in blks), dtype=torch.float32, device=v.device)
        _lib.call("geom_pool_features_ragged_fwd_f32", b, vt, v, vert_mesh, vert_list, cam_mat, cam_pos, n, blks, chans, dims, out, 0)
        ctx.save_for_backward(v, vert_mesh, vert_list, vert_off, cam_mat, cam_pos, *blks)
        ctx.meta = (chans, dims, n)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        v, vert_mesh, vert_list, vert_off, cam_mat, cam_pos = ctx.saved_tensors[:6]
        blks = ctx.saved_tensors[6:]
        chans, dims, n = ctx.meta
        vt, b = v.shape[0], cam_pos.shape[0]
        ctot = grad_out.shape[1]
        # the gradient in place when it is a column slice of a wider row-major buffer (the block's input gradient), else contiguous
        if grad_out.stride(1) == 1 and grad_out.stride(0) >= ctot and grad_out.is_cuda and grad_out.dtype == torch.float32:
            g, g_ld = grad_out, grad_out.stride(0)
        else:
            g, g_ld = grad_out.contiguous(), ctot
        need_blocks = [ctx.needs_input_grad[6 + i] for i in range(n)]
        gblks = [torch.empty_like(t) if need else None for t, need in zip(blks, need_blocks)]
        gverts = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        ws, ws_bytes = None, 0
        if any(need_blocks) or gverts is not None:
            ws_bytes = _lib.lib().geom_pool_features_ragged_bwd_workspace_bytes(b, vt, n, dims)
            ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=v.device)
        _lib.call("geom_pool_features_ragged_bwd_f32", b, vt, v, vert_mesh, vert_list, vert_off, cam_mat, cam_pos, n, blks, chans, dims,
                  g, g_ld if g_ld != ctot else 0, gblks, gverts, ws, ws_bytes)
        return (gverts, None, None, None, None, None) + tuple(gblks)


class PoolFeaturesProj(torch.autograd.Function):
    """PoolFeatures with the old driver's PROJECTION MATRICES in place of the camera pair (reference old_GEOMetrics/utils.py:379-427
    pooling(blocks, verts_pos, matrix)): proj [B,4,4] fp32, row-major, detached -- data, no gradient.  The same
    kernels' bodies instantiated for the matrix projection: one launch forward, two backward; headroom as PoolFeatures takes it."""

    @staticmethod
    def forward(ctx, verts, proj, headroom, *blocks):
        v = _f32(verts, "verts_pos", 3, 3)
        proj = _proj_matrices(proj, v.shape[0], v.device)
        blks, chans, dims, n, out, out_ld, front_args = _pool_forward_operands(v, headroom, blocks)
        b, nv, _ = v.shape
        _lib.call("geom_pool_features_proj_fwd_f32", b, nv, v, proj, n, blks, chans, dims, out, out_ld, *front_args)
        ctx.save_for_backward(v, proj, *blks)
        ctx.meta = (chans, dims, n)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        v, proj = ctx.saved_tensors[:2]
        blks = ctx.saved_tensors[2:]
        chans, dims, n = ctx.meta
        b, nv, _ = v.shape
        ctot = grad_out.shape[2]
        g, g_ld = _pitched_gradient(grad_out, grad_out.stride(0) == nv * grad_out.stride(1))
        need_blocks = [ctx.needs_input_grad[3 + i] for i in range(n)]
        gblks = [torch.empty_like(t) if need else None for t, need in zip(blks, need_blocks)]
        gverts = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        ws, ws_bytes = None, 0
        if any(need_blocks) or gverts is not None:       # (the camera route's workspace: the layout knows no camera)
            ws_bytes = _lib.lib().geom_pool_features_bwd_workspace_bytes(b, nv, n, dims)
            ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=v.device)
        _lib.call("geom_pool_features_proj_bwd_f32", b, nv, v, proj, n, blks, chans, dims, g, g_ld if g_ld != ctot else 0, gblks, gverts,
                  ws, ws_bytes)
        return (gverts, None, None) + tuple(gblks)


class RaggedPoolFeaturesProj(torch.autograd.Function):
    """RaggedPoolFeatures with proj [B,4,4] in place of the camera pair: row v of the [Vt, sum C] result is
    PoolFeaturesProj's row for vertex v as a vertex of mesh vert_mesh[v] alone, bit for bit."""

    @staticmethod
    def forward(ctx, verts, vert_mesh, vert_list, vert_off, proj, *blocks):
        v = _f32(verts, "verts_union", 2, 3)
        vert_mesh = _lib.require(vert_mesh, "vert_mesh", torch.int32, 1)
        vert_list = _lib.require(vert_list, "vert_list", torch.int32, 1)
        vert_off = _lib.require(vert_off, "vert_off", torch.int32, 1)
        blks = [_f32(b, "block", 4) for b in blocks]
        vt, b = v.shape[0], vert_off.shape[0] - 1
        proj = _proj_matrices(proj, b, v.device)
        if vt == 0 or b <= 0 or not blks:
            raise RuntimeError("the union must hold a vertex, the batch a mesh and a feature map (got %d vertices, %d meshes, %d maps)"
                               % (vt, b, len(blks)))
        if vert_mesh.shape[0] != vt or vert_list.shape[0] != vt:
            raise RuntimeError("vert_mesh and vert_list must hold one entry per vertex of the union (%d)" % vt)
        for blk in blks:
            if blk.shape[0] != b or blk.shape[2] != blk.shape[3]:
                raise RuntimeError("feature maps must be [B, C, dim, dim] with the matrices' batch size")
        n = len(blks)
        chans = (ctypes.c_int * n)(*[t.shape[1] for t in blks])
        dims = (ctypes.c_int * n)(*[t.shape[2] for t in blks])
        out = torch.empty(vt, sum(t.shape[1] for t in blks), dtype=torch.float32, device=v.device)
        _lib.call("geom_pool_features_ragged_proj_fwd_f32", b, vt, v, vert_mesh, vert_list, proj, n, blks, chans, dims, out, 0)
        ctx.save_for_backward(v, vert_mesh, vert_list, vert_off, proj, *blks)
        ctx.meta = (chans, dims, n)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        v, vert_mesh, vert_list, vert_off, proj = ctx.saved_tensors[:5]
        blks = ctx.saved_tensors[5:]
        chans, dims, n = ctx.meta
        vt, b = v.shape[0], proj.shape[0]
        ctot = grad_out.shape[1]
        g, g_ld = _pitched_gradient(grad_out, True)
        need_blocks = [ctx.needs_input_grad[5 + i] for i in range(n)]
        gblks = [torch.empty_like(t) if need else None for t, need in zip(blks, need_blocks)]
        gverts = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        ws, ws_bytes = None, 0
        if any(need_blocks) or gverts is not None:
            ws_bytes = _lib.lib().geom_pool_features_ragged_bwd_workspace_bytes(b, vt, n, dims)
            ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=v.device)
        _lib.call("geom_pool_features_ragged_proj_bwd_f32", b, vt, v, vert_mesh, vert_list, vert_off, proj, n, blks, chans, dims,
                  g, g_ld if g_ld != ctot else 0, gblks, gverts, ws, ws_bytes)
        return (gverts, None, None, None, None) + tuple(gblks)


def _proj_matrices(proj, b, device):
    """proj as the matrix launches take it: fp32 [b,4,4] on `device`, contiguous."""
    proj = _f32(proj, "the projection matrices", 3, 4)
    if tuple(proj.shape) != (b, 4, 4):
        raise RuntimeError("the projection matrices must be [B,4,4] with one matrix per mesh (got %s for %d meshes)" % (tuple(proj.shape), b))
    if proj.device != device:
        raise RuntimeError("the projection matrices live on %s, the vertices on %s" % (proj.device, device))
    return proj


class SegmentMax(torch.autograd.Function):
    """Column maximum per mesh of a ragged batch: x [sum(V), C], offsets [B+1] int64 (device) -> [B, C]
    (GCNMax's `torch.max(i_s, dim=0)[0]`, reference layers.py:78, for every mesh at once).  The gradient goes to
    the arg-max row only (lowest row on ties), written by a gather -- grad_x needs no zero fill."""

    @staticmethod
    def forward(ctx, x, offsets, max_len):
        x_ = _f32(x, "x", 2)
        offsets = _lib.require(offsets, "offsets", torch.int64, 1)
        nseg, c = offsets.numel() - 1, x_.shape[1]
        out = torch.empty(nseg, c, dtype=torch.float32, device=x_.device)
        arg = torch.empty(nseg, c, dtype=torch.int32, device=x_.device)
        ws_bytes = _lib.lib().geom_segment_max_workspace_bytes(nseg, c, int(max_len))
        ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=x_.device)
        _lib.call("geom_segment_max_fwd_f32", nseg, offsets, int(max_len), c, x_, out, arg, ws, ws_bytes)
        ctx.save_for_backward(offsets, arg)
        ctx.rows = x_.shape[0]
        ctx.mark_non_differentiable(arg)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        offsets, arg = ctx.saved_tensors
        g = grad_out.contiguous()
        nseg, c = arg.shape
        grad_x = torch.empty(ctx.rows, c, dtype=torch.float32, device=g.device)
        _lib.call("geom_segment_max_bwd_f32", nseg, offsets, ctx.rows, c, g, arg, grad_x)
        return grad_x, None, None


_rng_states = {}


def manual_seed(seed, device=None, mesh_offset=0):
    """(Re)seed the in-kernel sampler stream of `device` (default: current).  `mesh_offset` = the global index of
    the first mesh this process holds: the generator is keyed on (seed, stream position, global mesh index, sample),
    so data-parallel ranks that pass the same seed and their shard's offset draw exactly what one process holding the
    whole batch would draw.  Without a call the stream is seeded from torch's default generator the first time it is
    used, with a rank-distinct offset under torch.distributed.  One sampler stream per device: calls that draw
    from it must be issued on one HIP stream at a time (the position is advanced inside the kernel)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    state = torch.tensor([int(seed) & (2 ** 63 - 1), 0, 0, int(mesh_offset)], dtype=torch.int64).to(dev)   # seed, position, arrivals, first mesh
    _rng_states[key] = state
    return state


def set_rng_state(state, device=None):
    """Make `state` (a tensor manual_seed returned) the sampler stream of `device`: lets one process alternate
    between several independent streams (e.g. two shards stepped in turn)."""
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.int64 and tuple(state.shape) == (4,)):
        raise RuntimeError("set_rng_state: the state is a 4-element int64 tensor on a HIP device, as manual_seed returns it (got %s)"
                           % ("%s %s on %s" % (state.dtype, tuple(state.shape), state.device) if isinstance(state, torch.Tensor)
                              else type(state).__name__))
    dev = state.device if device is None else torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if state.device.index != key:
        raise RuntimeError("set_rng_state: the state is on %s, the stream it is set for on cuda:%d" % (state.device, key))
    _rng_states[key] = state


def _rng_state(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _rng_states.get(key)
    if st is None:
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        # ranks seeded alike (the reference seeds 41 everywhere) must not draw the same samples for different meshes
        st = manual_seed(torch.initial_seed() ^ 0x5DEECE66D, dev, mesh_offset=rank << 24)
    return st


def draw_samples(verts, faces, num, generator=None, with_points=False, prepare_scan_for=None, gt_index=None):
    """The random part of batch_sample (reference utils.py:604-612, 627-628): choices [B,num] ~
    area-weighted with replacement, u = sqrt(U1), v = U2, in ONE kernel: per-mesh face-area CDF in LDS (monotone by
    construction: a face of zero area is never drawn), binary search per sample, uniforms from an in-kernel Philox stream whose position lives on the device
    (graph replays draw fresh numbers; no generator bookkeeping launches).  With an explicit torch
    `generator` the uniforms come from torch.rand instead; meshes with more than 16384 faces take the
    torch.multinomial route.  with_points=True also returns the sampled points [B,num,3] (or None when the
    kernel could not produce them), which ops.SurfaceLoss accepts in place of its own gather launch.
    prepare_scan_for = n_gt (with with_points=True): the same launch also writes the triangle records of the surface scan
    of n_gt query points per mesh; a fifth return value is then the prepared workspace tensor (or None when the scan
    will not take the fused route), to be handed to ops.SurfaceLoss as `tri_ws`.  gt_index (an ops.GtIndex of the step's
    ground-truth clouds): the launch also lists the samples in a visiting order and writes their index for the culled
    Chamfer scan; the fifth return value is then an ops.ScanPrep carrying both."""
    verts_c = _f32(verts.detach(), "verts", 3, 3)
    faces = _lib.require(faces, "faces", torch.int64, 2, 3)
    b, nv, _ = verts_c.shape
    dev = verts_c.device
    choices = torch.empty(b, num, dtype=torch.int64, device=dev)
    u = torch.empty(b, num, dtype=torch.float32, device=dev)
    v = torch.empty(b, num, dtype=torch.float32, device=dev)
    uniforms = points = None
    if generator is None:
        if with_points:
            points = torch.empty(b, num, 3, dtype=torch.float32, device=dev)
        if with_points and prepare_scan_for:
            n_gt, nf = int(prepare_scan_for), faces.shape[0]
            ws_bytes = _lib.lib().geom_tri_distance_workspace_bytes(b, n_gt, nf)
            tri_ws = torch.empty(max(ws_bytes, 16) // 4, dtype=torch.float32, device=dev)
            prepared = ctypes.c_int(0)
            cull = s_index = None
            if gt_index is not None:
                s_index = torch.empty(max(int(_lib.lib().geom_nn_cull_index_floats(b, num)), 4), dtype=torch.float32, device=dev)
                cull = _lib.args(_lib.SurfaceCull, None, None, s_index, faces_in_order(verts_c, faces))
            code = _lib.status("geom_surface_prepare_f32", b, nv, verts_c, nf, faces, num, _rng_state(dev), choices, u, v, points,
                               n_gt, face_order(verts_c, faces), 0, tri_ws, ws_bytes, ctypes.byref(prepared), cull)
            if code == 0:
                if prepared.value & 2:
                    return choices, u, v, points, ScanPrep(tri_ws, s_index)
                return choices, u, v, points, (tri_ws if prepared.value else None)
        else:
            code = _lib.status("geom_draw_samples_rng_f32", b, nv, verts_c, faces.shape[0], faces, num, _rng_state(dev),
                               choices, u, v, points)
    else:
        uniforms = torch.rand(3, b, num, device=dev, generator=generator)
        code = _lib.status("geom_draw_samples_f32", b, nv, verts_c, faces.shape[0], faces, num, uniforms, choices, u, v)
    if code == _lib.EUNSUPPORTED:
        if uniforms is None:
            uniforms = torch.rand(3, b, num, device=dev)
        choices = torch.multinomial(face_areas(verts_c, faces), num, True, generator=generator)
        out = (choices, torch.sqrt(uniforms[1]), uniforms[2])
        if with_points:
            out = out + ((None, None) if prepare_scan_for else (None,))
        return out
    _lib.check(code, "geom_draw_samples_f32")
    if with_points:
        return (choices, u, v, points, None) if prepare_scan_for else (choices, u, v, points)
    return choices, u, v


# ------------------------------------- ragged batches: every mesh owns its faces ----
def _ragged_mesh(verts, faces, face_list, face_off):
    """The checked union mesh of a ragged batch: (verts [Vt,3] fp32, faces [Ft,3] int64, face_list int32 [Ft], face_off int32
    [B+1]) contiguous on one device, and B."""
    verts = _f32(verts.detach(), "verts", 2, 3)
    faces = _lib.require(faces, "faces", torch.int64, 2, 3)
    face_list = _lib.require(face_list, "face_list", torch.int32, 1)
    face_off = _lib.require(face_off, "face_off", torch.int32, 1)
    _lib.same_device(verts, faces, face_list, face_off)
    if face_list.numel() != faces.shape[0] or face_off.numel() < 1:
        raise RuntimeError("face_list must list the %d faces and face_off hold B+1 offsets (ragged.group_faces)" % faces.shape[0])
    return verts, faces, face_list, face_off, face_off.numel() - 1


def draw_samples_ragged(verts, faces, face_list, face_off, num, generator=None, with_points=False):
    """draw_samples for a ragged batch (verts [Vt,3] the union, face_list / face_off from ragged.group_faces): `num` samples
    per mesh from its OWN faces, choices [B,num] UNION face ids, u = sqrt(U1), v = U2 -- per mesh exactly what draw_samples
    draws for that mesh's faces as mesh m of a batch of B, from the same in-kernel stream (or torch.rand uniforms with an
    explicit `generator`).  One launch, no host read.  A mesh with no face or more than 16384 gets a valid face id and NaN
    u / v / points (its face count is known on the device only): a loss on them is NaN, nothing indexes out of range."""
    verts, faces, face_list, face_off, b = _ragged_mesh(verts, faces, face_list, face_off)
    dev = verts.device
    choices = torch.empty(b, num, dtype=torch.int64, device=dev)
    u = torch.empty(b, num, dtype=torch.float32, device=dev)
    v = torch.empty(b, num, dtype=torch.float32, device=dev)
    points = torch.empty(b, num, 3, dtype=torch.float32, device=dev) if with_points else None
    uniforms = None if generator is None else torch.rand(3, b, num, device=dev, generator=generator)
    _lib.call("geom_draw_samples_ragged_f32", b, verts.shape[0], verts, faces.shape[0], faces, face_list, face_off, num, uniforms,
              _rng_state(dev) if generator is None else None, choices, u, v, points)
    return (choices, u, v, points) if with_points else (choices, u, v)


def tri_distance_ragged(xyz, verts, faces, face_list, face_off, flags=None):
    """(dist [B,N] fp32, point [B,N] int32 region codes, index [B,N] int32 UNION face ids): the closest triangle of every query
    xyz[m] among the faces of mesh m only -- per mesh the bits of tri_distance_indexed on that mesh alone.  The workspace-free
    culled scan (_lib.FLAG_TRI_BRUTE_FORCE: every pair).  A mesh without faces: (NaN, 0, 0)."""
    xyz = _f32(xyz.detach(), "xyz", 3, 3)
    verts, faces, face_list, face_off, b = _ragged_mesh(verts, faces, face_list, face_off)
    if xyz.shape[0] != b or xyz.device != verts.device:
        raise RuntimeError("xyz must be [B,N,3] on the meshes' device with B = %d meshes" % b)
    n, dev = xyz.shape[1], xyz.device
    dist = torch.empty(b, n, dtype=torch.float32, device=dev)
    point = torch.empty(b, n, dtype=torch.int32, device=dev)
    index = torch.empty(b, n, dtype=torch.int32, device=dev)
    _lib.call("geom_tri_distance_ragged_f32", b, n, xyz, verts.shape[0], verts, faces.shape[0], faces, face_list, face_off, dist,
              point, index, _lib.quirk_flags() if flags is None else flags)
    return dist, point, index


_row_offsets = {}     # (device, rows, stride) -> int32 [rows,1] = row * stride


def _offsets_by_row(rows, stride, dev):
    """int32 [rows,1] holding row * stride: what turns per-mesh indices [B,n] into indices of the flattened batch."""
    make = lambda: (torch.arange(rows, dtype=torch.int32, device=dev) * stride).view(rows, 1)
    if torch.cuda.is_current_stream_capturing():      # (memory made during a capture belongs to the graph: never kept)
        return make()
    key = (dev, rows, stride)
    if key not in _row_offsets:
        _row_offsets[key] = make()
    return _row_offsets[key]


# The backward of the ragged surface loss: "ordered" (the default: finalize + gather, no float atomics, same bits on every run)
# or "scatter" (GEOM_RAGGED_BACKWARD=scatter: the fp32-atomic kernels, always -- the A/B switch; they also serve a batch whose
# points per mesh do not fit the finalize launch's LDS).
ragged_backward = os.environ.get("GEOM_RAGGED_BACKWARD", "ordered")


def _face_positions(face_list, face_off):
    """ragged.face_positions from the grouping alone: the inverse of face_list, -1 outside [face_off[0], face_off[B])."""
    pos = torch.empty_like(face_list)
    pos[face_list.to(torch.int64)] = torch.arange(face_list.numel(), dtype=torch.int32, device=face_list.device)
    return torch.where((pos >= face_off[0]) & (pos < face_off[-1]), pos, torch.full_like(pos, -1))


class RaggedSurfaceLoss(torch.autograd.Function):
    """SurfaceLoss for a ragged batch: B meshes with their own faces on one union vertex array, one call instead of B.

    Value: the mean over the meshes of what SurfaceLoss gives for that mesh alone -- scale * (sum sq_pred / (B num) +
    sum sq_other / (B N)); with mesh_weight [B] fp32, (1/B) sum_m w[m] * (mesh m's loss).  Only the steps that must know which
    faces belong to which mesh run on the ragged kernels (the draw: ops.draw_samples_ragged, the point-to-triangle scan, and
    the backward's preparation); everything else sees either regular [B, ., 3] clouds (the Chamfer scan at b = B) or the union
    as ONE mesh at b = 1 with the union's face ids (gather of the points, closest point).
    Backward: SurfaceLoss's -- when a gradient is wanted the forward ends with the ragged finalize launch (every mesh's points
    counting-sorted by face in ascending id order, csrc/surface_gather.hip) and the backward is ONE gather launch over the
    union's vertices: no zero-fill, no float atomics, the same bits on every run, per mesh the bits of the batched pair on that
    mesh alone.  face_pos: ragged.face_positions (None: derived from the grouping).  Where the points of a mesh do not fit the
    finalize launch's LDS (num + N beyond ~38 000), or with ragged_backward = "scatter": the fp32-atomic scatter kernels of
    SurfaceLoss's overflow fallback, which know no per-mesh weights (a RuntimeError with them).  No host read."""

    @staticmethod
    def forward(ctx, verts, faces, face_list, face_off, gt, choices, u, v, two_sided, scale, points=None, need_gt_nn=True,
                mesh_weight=None, face_pos=None):
        verts_c, faces, face_list, face_off, b = _ragged_mesh(verts, faces, face_list, face_off)
        if mesh_weight is not None:
            mesh_weight = _f32(mesh_weight.detach(), "mesh_weight", 1)
            if mesh_weight.shape[0] != b or mesh_weight.device != verts_c.device:
                raise RuntimeError("mesh_weight must be [B] on the meshes' device")
        gt_c = _f32(gt.detach(), "gt_points", 3, 3)
        if gt_c.shape[0] != b or gt_c.device != verts_c.device:
            raise RuntimeError("gt_points must be [B,N,3] on the meshes' device with B = %d meshes" % b)
        choices = _lib.require(choices.reshape(b, -1), "choices", torch.int64, 2)
        u, v = _f32(u.reshape(b, -1), "u", 2), _f32(v.reshape(b, -1), "v", 2)
        if u.shape != choices.shape or v.shape != choices.shape:
            raise RuntimeError("choices/u/v must all be [B,num]")
        nv, nf, num, n_gt, dev = verts_c.shape[0], faces.shape[0], choices.shape[1], gt_c.shape[1], verts_c.device
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        if points is None:      # replayed draws: the union is one mesh of B * num samples
            points = torch.empty(b, num, 3, **f32)
            _lib.call("geom_sample_faces_fwd_f32", 1, nv, verts_c, nf, faces, b * num, choices, u, v, points)
        else:
            points = _f32(points.detach(), "points", 3, 3)
            if points.shape != (b, num, 3):
                raise RuntimeError("points must be [B,num,3] for the given draws")
        flags = _chamfer.default_flags()
        if flags & _lib.FLAG_REF_TAIL_TRUNC:
            raise RuntimeError("the ragged surface loss has no reference-quirk mode (set_reference_quirks(False))")
        # Chamfer: samples and gt are regular clouds per mesh; the gt points' direction only where something reads it
        one_dir = not need_gt_nn and not two_sided
        sq_pred, idx_g = torch.empty(b, num, **f32), torch.empty(b, num, **i32)
        sq_gt, idx_p = (None, None) if one_dir else (torch.empty(b, n_gt, **f32), torch.empty(b, n_gt, **i32))
        _lib.call("geom_chamfer_nn_f32", b, n_gt, gt_c, num, points, sq_gt, idx_p, sq_pred, idx_g,
                  flags | (_lib.FLAG_NN_SAMPLES_ONLY if one_dir else 0))
        if two_sided:
            other_sq = sq_gt
        else:                   # every gt point against the faces of ITS mesh, then the closest point on the winner (b = 1)
            option, index = torch.empty(b, n_gt, **i32), torch.empty(b, n_gt, **i32)
            other_sq, closest, weights = torch.empty(b, n_gt, **f32), torch.empty(b, n_gt, 3, **f32), torch.empty(b, n_gt, 3, **f32)
            _lib.call("geom_tri_distance_ragged_f32", b, n_gt, gt_c, nv, verts_c, nf, faces, face_list, face_off,
                      torch.empty(b, n_gt, **f32), option, index, 0)
            _lib.call("geom_p2tri_loss_fwd_f32", 1, b * n_gt, gt_c, nv, verts_c, nf, faces, option, index, other_sq, closest, weights)
        out = torch.empty((), **f32)
        if mesh_weight is None:         # (the value keeps these three sums whichever backward follows)
            parts = torch.empty(2, **f32)
            _lib.call("geom_sum_f32", sq_pred.numel(), sq_pred, scale / sq_pred.numel(), parts)
            _lib.call("geom_sum_f32", other_sq.numel(), other_sq, scale / other_sq.numel(), parts[1:])
            _lib.call("geom_sum_f32", 2, parts, 1.0, out)
        want = bool(ctx.needs_input_grad[0])
        # the ordered backward's preparation; with per-mesh weights the same launch's loss role forms the weighted loss
        ctx.order = None
        if mesh_weight is not None and ragged_backward == "scatter":
            raise RuntimeError("per-mesh weights need the ordered backward (GEOM_RAGGED_BACKWARD=scatter is set)")
        if mesh_weight is not None or (want and ragged_backward != "scatter"):
            if face_pos is None:
                face_pos = _face_positions(face_list, face_off)
            face_pos = _lib.require(face_pos, "face_pos", torch.int32, 1)
            if face_pos.numel() != nf or face_pos.device != dev:
                raise RuntimeError("face_pos must hold one position per face on the meshes' device (ragged.face_positions)")
            order = torch.empty(_lib.lib().geom_surface_order_ragged_words(b, nf, num, n_gt), dtype=torch.int32, device=dev)
            code = _lib.status("geom_surface_finalize_ragged_f32", b, nf, face_list, face_off, face_pos, num, choices, u, v, points,
                               n_gt, gt_c, idx_g, idx_p if two_sided else None, None if two_sided else index,
                               None if two_sided else closest, None if two_sided else weights, sq_pred, other_sq,
                               scale / sq_pred.numel(), scale / other_sq.numel(), scale / (b * num), scale / (b * n_gt), order,
                               None if mesh_weight is None else out, mesh_weight)
            if code == _lib.EUNSUPPORTED and mesh_weight is not None:
                raise RuntimeError("per-mesh weights need the ordered backward (the points of a mesh within ~38 000)")
            if code != _lib.EUNSUPPORTED:       # (else: too many points per mesh for the in-LDS ordering -- scatter backward)
                _lib.check(code, "geom_surface_finalize_ragged_f32")
                if want:
                    from . import ragged
                    ctx.order, ctx.vf, ctx.mesh_weight = order, ragged.vertex_faces(faces, nv), mesh_weight
                    ctx.shape = (b, num, n_gt, nf)
        if scan_capture is not None:
            scan_capture.update(idx_gt=idx_p, idx_pred=idx_g, sq_gt=sq_gt, sq_pred=sq_pred, choices=choices, u=u, v=v, points=points)
            if not two_sided:
                scan_capture.update(tri_index=index, tri_option=option, closest=closest, weights=weights, sq=other_sq)
        if want and ctx.order is None:  # the scatter backward sees ONE mesh: per-mesh neighbour indices become indices of the flat batch
            idx_g_flat = idx_g + _offsets_by_row(b, n_gt, dev)
            if two_sided:
                ctx.save_for_backward(faces, choices, u, v, points, gt_c, idx_g_flat, idx_p + _offsets_by_row(b, num, dev))
            else:
                ctx.save_for_backward(faces, choices, u, v, points, gt_c, idx_g_flat, index, closest, weights)
        ctx.two_sided, ctx.scale, ctx.nv = two_sided, scale, nv
        ctx.mark_non_differentiable(*(t for t in (sq_gt, sq_pred) if t is not None))
        ctx.set_materialize_grads(False)
        return out, sq_gt, sq_pred

    @staticmethod
    def backward(ctx, grad, _g1, _g2):
        grad = grad.contiguous()
        if ctx.order is not None:           # prepared by the forward's finalize launch: one gather, no atomics
            b, num, n_gt, nf = ctx.shape
            grad_verts = torch.empty(ctx.nv, 3, dtype=torch.float32, device=ctx.order.device)
            _lib.call("geom_surface_gather_ragged_f32", b, ctx.nv, nf, ctx.vf[0], ctx.vf[1], num, n_gt, ctx.order, grad,
                      ctx.mesh_weight, grad_verts)
            return (grad_verts,) + (None,) * 13
        saved = ctx.saved_tensors
        faces, choices, u, v, points, gt, idx_g = saved[:7]
        b, num, _ = points.shape
        n_gt, nf, nv = gt.shape[1], faces.shape[0], ctx.nv
        grad_verts = torch.zeros(nv, 3, dtype=torch.float32, device=points.device)
        coef_s, coef_o = ctx.scale / (b * num), ctx.scale / (b * n_gt)
        if ctx.two_sided:
            for other_idx, via_nn, coef in ((idx_g, 0, coef_s), (saved[7], 1, coef_o)):
                _lib.call("geom_sample_chamfer_bwd_f32", 1, nv, nf, faces, b * num, choices, u, v, points, b * n_gt, gt, other_idx,
                          via_nn, grad, coef, grad_verts)
        else:
            index, closest, weights = saved[7:10]
            _lib.call("geom_surface_loss_bwd_f32", 1, nv, nf, faces, b * num, choices, u, v, points, b * n_gt, gt, idx_g, index,
                      closest, weights, grad, coef_s, coef_o, grad_verts)
        return (grad_verts,) + (None,) * 13


class VertexHead(torch.autograd.Function):
    """pos = base + scale * feat[..., :3] in one kernel; the adjoint writes grad_feat = [scale*grad_pos | 0]
    in one pass (a slice + mul + add costs two launches forward and mul + zero-fill + strided copy backward)."""

    @staticmethod
    def forward(ctx, base, feat, scale):
        b_ = _f32(base, "base", 3, 3)
        f_ = _f32(feat, "feat", 3)
        if f_.shape[:2] != b_.shape[:2] or f_.shape[2] < 4 or f_.shape[2] % 4:
            raise RuntimeError("feat must be [B,V,C] with C a multiple of 4 matching base [B,V,3]")
        pos = torch.empty_like(b_)
        rows = b_.shape[0] * b_.shape[1]
        _lib.call("geom_vertex_head_fwd_f32", rows, f_.shape[2], b_, f_, float(scale), pos)
        ctx.scale, ctx.c = float(scale), f_.shape[2]
        return pos

    @staticmethod
    def backward(ctx, grad_pos):
        g = grad_pos.contiguous()
        rows = g.shape[0] * g.shape[1]
        grad_feat = None
        if ctx.needs_input_grad[1]:
            grad_feat = torch.empty(g.shape[0], g.shape[1], ctx.c, dtype=torch.float32, device=g.device)
            _lib.call("geom_vertex_head_bwd_f32", rows, ctx.c, g, ctx.scale, grad_feat)
        return (g if ctx.needs_input_grad[0] else None), grad_feat, None


__all__ = ["face_areas", "device_sum", "SampleFaces", "GatherSqDistSum", "PointToTriangleSum", "SurfaceLoss",
           "Laplacian", "EdgeSqLenSum", "PoolFeatures", "RaggedPoolFeatures", "PoolFeaturesProj", "RaggedPoolFeaturesProj",
           "VertexHead", "SegmentMax", "manual_seed", "set_rng_state",
           "draw_samples", "GtIndex", "ScanPrep", "RaggedSurfaceLoss", "draw_samples_ragged", "tri_distance_ragged",
           "chamfer_nn", "tri_distance_indexed"]


# ---------------------------------------------- adaptive face splitting (csrc/face_split.hip) ----
def face_curvature(verts, faces, face_list):
    """curvature [Fa] in radians of the active faces of ONE mesh (reference old_GEOMetrics/utils.py:431-465): one launch."""
    v = _f32(verts.detach(), "verts", 2, 3)
    faces = _lib.require(faces, "faces", torch.int64, 2, 3)
    face_list = _lib.require(face_list, "face_list", torch.int64, 3, 3)
    out = torch.empty(face_list.shape[0], dtype=torch.float32, device=v.device)
    _lib.call("geom_face_curvature_f32", v.shape[0], v, faces.shape[0], faces, face_list.shape[0], face_list, out)
    return out


def select_faces(curvature, angle):
    """(selected [Fa] int64 -- its first `count` entries are the positions with (c * 180) / pi > angle, ascending --, count_top3
    [4] int64 = {count, the positions of the three largest curvatures}), both on the device: one launch, no host read."""
    c = _f32(curvature, "curvature", 1)
    selected = torch.empty(c.shape[0], dtype=torch.int64, device=c.device)
    count_top3 = torch.empty(4, dtype=torch.int64, device=c.device)
    _lib.call("geom_face_select_f32", c.shape[0], c, float(angle), selected, count_top3)
    return selected, count_top3


class SplitIndex:
    """The index tables of one split, all int64 on the device and made without a host read (geom_hip.h, geom_face_split_index):
    corners [S,3], split_pos / unsplit_rank [Fa], face_s [Ft], and the vertex -> split-face incidence inc_ptr [V+1] /
    inc_item [3S] (per vertex the split faces it is a corner of, ascending) that the adjacency rows and the vertices'
    backward both walk."""
    __slots__ = ("s", "nv", "corners", "split_pos", "unsplit_rank", "face_s", "inc_ptr", "inc_item")


def split_index(faces, face_list, splitting, nv):
    """SplitIndex of splitting the active rows `splitting` (unique positions into face_list): one launch of one workgroup
    (geom_face_split_index: scatters, two running sums, the incidence rows filled and sorted in place), no host read."""
    ix = SplitIndex()
    dev = faces.device
    s = ix.s = int(splitting.numel())
    ix.nv = int(nv)
    new = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
    ix.corners, ix.split_pos, ix.unsplit_rank, ix.face_s = new(s, 3), new(face_list.shape[0]), new(face_list.shape[0]), new(faces.shape[0])
    ix.inc_ptr, ix.inc_item = new(ix.nv + 1), new(3 * s)
    cursor = new(ix.nv)
    _lib.call("geom_face_split_index", ix.nv, faces.shape[0], faces, face_list.shape[0], face_list, s, splitting, ix.corners,
              ix.split_pos, ix.unsplit_rank, ix.face_s, ix.inc_ptr, ix.inc_item, cursor)
    return ix


def split_tables(faces, face_list, ix, rowptr, col, dense=True):
    """Everything geom_face_split_tables writes, in one launch: dict of new_faces, new_face_list, rowptr, col, val, val_t, ones
    and (dense) the two [V+S,V+S] matrices adj / adj_orig, zero-filled here and given their non-zeros by the launch."""
    dev = faces.device
    nv, s, nft, nfa, nnz = ix.nv, ix.s, faces.shape[0], face_list.shape[0], col.numel()
    n, nnz_new = nv + s, nnz + 7 * s
    out = {"new_faces": torch.empty(nft + 3 * s, 3, dtype=torch.int64, device=dev),
           "new_face_list": torch.empty(nfa + 2 * s, 3, 3, dtype=torch.int64, device=dev),
           "rowptr": torch.empty(n + 1, dtype=torch.int32, device=dev), "col": torch.empty(nnz_new, dtype=torch.int32, device=dev),
           "val": torch.empty(nnz_new, dtype=torch.float32, device=dev), "val_t": torch.empty(nnz_new, dtype=torch.float32, device=dev),
           "ones": torch.empty(nnz_new, dtype=torch.float32, device=dev),
           "adj": torch.zeros(n, n, dtype=torch.float32, device=dev) if dense else None,
           "adj_orig": torch.zeros(n, n, dtype=torch.float32, device=dev) if dense else None}
    args = _lib.args(_lib.FaceSplit, nv, nft, nfa, s, nnz, faces, face_list, ix.corners, ix.split_pos, ix.unsplit_rank,
                     ix.face_s, ix.inc_ptr, ix.inc_item, rowptr, col, out["new_faces"], out["new_face_list"], out["rowptr"],
                     out["col"], out["val"], out["val_t"], out["ones"], out["adj"], out["adj_orig"])
    _lib.call("geom_face_split_tables", args)
    return out


class SplitVertices(torch.autograd.Function):
    """(verts [V,3], features [V,C]) -> ([V+S,3], [V+S,C]): old rows copied, row V + k the mean (x/3 + y/3) + z/3 of the corners
    of split face k (reference old_GEOMetrics/utils.py:590-596); one launch per direction, the backward a gather over the
    SplitIndex's incidence table (no atomics: bit-reproducible)."""

    @staticmethod
    def forward(ctx, verts, features, ix):
        v, f = _f32(verts, "verts", 2, 3), _f32(features, "features", 2)
        if f.shape[0] != v.shape[0] or v.shape[0] != ix.nv:
            raise RuntimeError("verts %s and features %s must both have the %d rows of the mesh" % (tuple(v.shape), tuple(f.shape), ix.nv))
        out_v = torch.empty(ix.nv + ix.s, 3, dtype=torch.float32, device=v.device)
        out_f = torch.empty(ix.nv + ix.s, f.shape[1], dtype=torch.float32, device=v.device)
        _lib.call("geom_split_vertices_fwd_f32", ix.nv, ix.s, f.shape[1], v, f, ix.corners, out_v, out_f)
        ctx.ix, ctx.c = ix, f.shape[1]
        return out_v, out_f

    @staticmethod
    def backward(ctx, grad_v, grad_f):
        ix = ctx.ix
        gv, gf = grad_v.contiguous(), grad_f.contiguous()
        out_v = torch.empty(ix.nv, 3, dtype=torch.float32, device=gv.device)
        out_f = torch.empty(ix.nv, ctx.c, dtype=torch.float32, device=gv.device)
        _lib.call("geom_split_vertices_bwd_f32", ix.nv, ix.s, ctx.c, gv, gf, ix.inc_ptr, ix.inc_item, out_v, out_f)
        return out_v, out_f, None


# ---------------------------------------------- the same for the union of a ragged batch ----
def select_faces_ragged(curvature, angle, row_list, row_off):
    """The selection of select_faces per mesh (geom_face_select_ragged_f32; row_list / row_off: ragged.group_rows): (selected
    int64 [Fa + 3 b] -- its first totals[0] entries are mesh 0's positions, then mesh 1's, ... --, counts int64 [b], totals int64
    [2] = {entries, meshes without three faces that have a curvature}), all on the device: two launches, no host read."""
    c = _f32(curvature, "curvature", 1)
    row_list = _lib.require(row_list, "row_list", torch.int32, 1)
    row_off = _lib.require(row_off, "row_off", torch.int32, 1)
    _lib.same_device(c, row_list, row_off)
    b = row_off.numel() - 1
    if row_list.numel() != c.shape[0] or b < 0:
        raise RuntimeError("row_list must list the %d active rows and row_off hold b+1 offsets (ragged.group_rows)" % c.shape[0])
    new = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=c.device)
    stats, selected, counts, totals = new(b, 4), new(c.shape[0] + 3 * b), new(b), new(2)
    _lib.call("geom_face_select_ragged_f32", c.shape[0], c, float(angle), b, row_list, row_off, stats, selected, counts, totals)
    return selected, counts, totals


def split_index_ragged(faces, face_list, splitting, nv, vert_mesh, face_mesh):
    """(SplitIndex, vert_mesh_new int64 [V+S], face_mesh_new int64 [Ft+3S]) of splitting the active rows `splitting` of a union:
    the tables of split_index made by geom_face_split_index_ragged -- a zero-fill and at most four launches over chunks of the
    union, no host read -- and the mesh ids after the split."""
    ix = SplitIndex()
    dev = faces.device
    s = ix.s = int(splitting.numel())
    ix.nv = int(nv)
    nft, nfa = faces.shape[0], face_list.shape[0]
    new = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
    ix.corners, ix.split_pos, ix.unsplit_rank, ix.face_s = new(s, 3), new(nfa), new(nfa), new(nft)
    ix.inc_ptr, ix.inc_item = new(ix.nv + 1), new(3 * s)
    vert_mesh_new, face_mesh_new = new(ix.nv + s), new(nft + 3 * s)
    workspace = new(max(int(_lib.lib().geom_face_split_index_ragged_words(ix.nv, nft, nfa, s)), 1))
    _lib.call("geom_face_split_index_ragged", ix.nv, nft, faces, nfa, face_list, s, splitting, vert_mesh, face_mesh, ix.corners,
              ix.split_pos, ix.unsplit_rank, ix.face_s, ix.inc_ptr, ix.inc_item, vert_mesh_new, face_mesh_new, workspace)
    return ix, vert_mesh_new, face_mesh_new
