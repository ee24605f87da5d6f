"""Drop-in for the reference package `tri_distance` (tri_distance/tri_distance.py:9-43).

    TriDistance()(xyz1, tri1, tri2, tri3) -> (dist, point, index)

dist [B,N] f32 squared distance to the chosen closest point, point [B,N] i32 region code 0..6,
index [B,N] i32 winning triangle; all non-differentiable like the reference's.
`tri_distance_indexed` takes (verts, faces) and gathers the corners in-kernel.

`order`: an int32 permutation of the triangles that makes neighbours in the list neighbours in space
switches the scan to its two-level form (groups of 16 triangles under a group sphere).  It never changes
the result.  `tri_distance_indexed` derives a k-d tree leaf order of the face centroids once per face list
(`face_order`, cached on the tensor's identity -- mesh deformation keeps a topology's order coherent);
`morton_order` is the device-only alternative.
"""
import torch

from .. import _lib
from .._identity import ByTensor

_order_cache = ByTensor()   # faces -> [visiting order, the faces in that order (made when first asked for)]


def morton_order(centroids):
    """int32 permutation sorting [M,3] points along a 30-bit Morton (Z-order) curve of their bounding box."""
    c = torch.nan_to_num(centroids.detach().to(torch.float32), nan=0.0, posinf=0.0, neginf=0.0)
    lo = c.amin(0)
    span = (c.amax(0) - lo).clamp_min(1e-30)
    q = ((c - lo) / span * 1023.0).to(torch.int64).clamp_(0, 1023)

    def spread(x):          # 10 bits -> every third bit
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249

    code = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    return torch.argsort(code, stable=True).to(torch.int32).contiguous()


def kd_order(centroids, leaf=16):
    """int32 permutation that lists [M,3] points leaf by leaf of a median-split k-d tree (split along the longest
    axis of the node's bounding box, at a multiple of `leaf`): every run of `leaf` consecutive entries is one compact
    cell -- the property the two-level scan's groups need.  Measured on the 5120-face BASELINE mesh the group spheres
    come out 25 % smaller than along a 30-bit Morton curve.  Host-side, once per face list (numpy; one device->host
    copy)."""
    import numpy as np
    c = np.nan_to_num(centroids.detach().to(torch.float32).cpu().numpy(), nan=0.0, posinf=0.0, neginf=0.0)
    order = np.arange(c.shape[0])
    nodes = [(0, c.shape[0])]
    while nodes:
        nxt = []
        for a, b in nodes:
            n = b - a
            if n <= leaf:
                continue
            idx = order[a:b]
            pts = c[idx]
            axis = int(np.argmax(pts.max(0) - pts.min(0)))
            order[a:b] = idx[np.argsort(pts[:, axis], kind="stable")]
            half = ((n // leaf + 1) // 2) * leaf          # left child: a whole number of leaves
            nxt += [(a, a + half), (a + half, b)]
        nodes = nxt
    return torch.from_numpy(order.astype(np.int32)).to(centroids.device)


def face_order(verts, faces):
    """Coherent visiting order of `faces` [F,3], from the centroids of the first mesh of `verts` [B,V,3] the
    face list is seen with; cached per faces TENSOR OBJECT and in-place version (_identity.ByTensor)."""
    hit = _order_cache.get(faces)
    if hit is not None:
        return hit[0]
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        return None
    with torch.no_grad():
        order = kd_order(verts[0][faces].mean(dim=1))
    return _order_cache.put([order, None], faces)[0]


def faces_in_order(verts, faces):
    """int32 [F,3]: faces[face_order] -- the corners of the face at every position of the visiting order (cached with the
    order; None when there is none).  The sorted draws of the surface step read their corners from it."""
    order = face_order(verts, faces)
    if order is None:
        return None
    hit = _order_cache.get(faces)
    if hit[1] is None:
        hit[1] = faces[order.long()].to(torch.int32).contiguous()
    return hit[1]


# ---- the reference-shaped entry (tri1 / tri2 / tri3 corner tensors, tri_distance.py:9-43): no face list to key a cache on --
# the corner tensors are fresh gathers every step (utils.py:467-470).  What stays the same from call to call is the TOPOLOGY
# behind them, and mesh deformation keeps a topology's visiting order coherent; so one order is kept per (triangle count,
# device) and rebuilt on the device (Morton curve of the first mesh's centroids: a dozen small launches, no host
# synchronisation) every SOUP_REFRESH calls -- a stale or foreign order can only cost speed, never change a result
# (the scan's keys carry the original triangle index).
SOUP_REFRESH = 256
_soup_orders = {}   # (m, device) -> [order, calls since it was built, handed out during a stream capture]


def soup_order(tri1, tri2, tri3):
    """Visiting order for a [B,M,3] x 3 triangle soup (see above); None while a HIP graph is being captured before any
    order exists (the flat scan then serves the call).  An order that was handed out DURING a capture is never replaced:
    the graph has its address baked in, and a refreshed entry would free the memory its replays read (the prep kernel
    drops out-of-range entries, so triangles would silently go missing from the arg-min)."""
    m = tri1.shape[1]
    if tri1.shape[0] == 0 or m < 64:
        return None
    key = (m, tri1.device)
    hit = _soup_orders.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if hit is not None and (hit[1] < SOUP_REFRESH or capturing or hit[2]):
        hit[1] += 1
        hit[2] = hit[2] or capturing
        return hit[0]
    if capturing:
        return None
    with torch.no_grad():
        order = morton_order((tri1[0] + tri2[0] + tri3[0]) * (1.0 / 3.0))
    _soup_orders[key] = [order, 1, False]
    return order


def _checked_order(order, m, dev):
    if order is None:
        return None
    order = _lib.require(order, "order", torch.int32, 1)
    if order.numel() != m or order.device != dev:
        raise RuntimeError("order must be an int32 permutation of the %d triangles on %s" % (m, dev))
    return order


def _outputs(b, n, dev):
    return (torch.empty(b, n, dtype=torch.float32, device=dev),
            torch.empty(b, n, dtype=torch.int32, device=dev),
            torch.empty(b, n, dtype=torch.int32, device=dev))


def _workspace(b, n, m, dev):
    """Scratch for the per-triangle {sphere, corners} records (64 B per triangle); torch's caching
    allocator makes this free after the first call and keeps it hipGraph-capturable."""
    nbytes = _lib.lib().geom_tri_distance_workspace_bytes(b, n, m)
    return torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=dev), nbytes


def _scan(names, xyz1, m, geometry, outputs, flags, use_workspace, order):
    """One launch of a tri scan.  names: (workspace entry point, workspace-free one); geometry: the entry point's arguments
    between xyz and order (the three corner arrays, or nv / verts / nf / faces); outputs: (dist, point, index)."""
    b, n, _ = xyz1.shape
    dev = xyz1.device
    if use_workspace:
        ws, nbytes = _workspace(b, n, m, dev)
        code = _lib.status(names[0], b, n, xyz1, *geometry, _checked_order(order, m, dev), *outputs, flags, ws, nbytes)
    else:
        code = _lib.status(names[1], b, n, xyz1, *geometry, *outputs, flags)
    _lib.check(code, names[1])


def forward_cuda(xyz1, tri1, tri2, tri3, dist, point, index, flags=None, use_workspace=True, order=None):
    """Same call shape as the reference's pybind `tri.forward_cuda` (tri_distance.cpp:16-30,34-36)."""
    if flags is None:
        flags = _lib.quirk_flags()
    m = tri1.shape[1]
    _scan(("geom_tri_distance_ws_f32", "geom_tri_distance_f32"), xyz1, m,
          (m, tri1, tri2, tri3), (dist, point, index), flags, use_workspace, order)


def tri_distance(xyz1, tri1, tri2, tri3, flags=None, use_workspace=True, order="auto"):
    """flags: None = the package default (0, or GEOM_FLAG_REF_TAIL_TRUNC in reference-quirk mode:
    geometrics_amd.set_reference_quirks / GEOM_REF_QUIRKS).
    order: "auto" (cached Morton order of the triangle centroids -> two-level scan, see soup_order), None (flat scan)
    or an explicit int32 permutation of the triangles."""
    xyz1 = _lib.require(xyz1.detach(), "xyz1", torch.float32, 3, 3)
    tris = [_lib.require(t.detach(), "tri%d" % (i + 1), torch.float32, 3, 3) for i, t in enumerate((tri1, tri2, tri3))]
    dev = _lib.same_device(xyz1, *tris)
    b, n, _ = xyz1.shape
    for t in tris:
        if t.shape != tris[0].shape or t.shape[0] != b:
            raise RuntimeError("tri1/tri2/tri3 must share one [B,M,3] shape with xyz1's batch")
    outputs = _outputs(b, n, dev)
    if isinstance(order, str):
        order = soup_order(*tris) if use_workspace else None
    forward_cuda(xyz1, tris[0], tris[1], tris[2], *outputs, flags, use_workspace, order)
    return outputs


def tri_distance_indexed(xyz1, verts, faces, flags=None, use_workspace=True, order="auto"):
    """Corners gathered in-kernel from verts [B,V,3] through faces [F,3] (int64).  flags: None = the package default (see
    tri_distance).  order: "auto" (cached k-d leaf
    order of the face centroids -> two-level scan), None (flat scan) or an explicit int32 permutation."""
    xyz1 = _lib.require(xyz1.detach(), "xyz1", torch.float32, 3, 3)
    verts = _lib.require(verts.detach(), "verts", torch.float32, 3, 3)
    faces = _lib.require(faces, "faces", torch.int64, 2, 3)
    dev = _lib.same_device(xyz1, verts, faces)
    b, n, _ = xyz1.shape
    if verts.shape[0] != b:
        raise RuntimeError("verts and xyz1 batch sizes differ")
    if flags is None:
        flags = _lib.quirk_flags()
    outputs = _outputs(b, n, dev)
    if use_workspace and isinstance(order, str):
        order = face_order(verts, faces)
    _scan(("geom_tri_distance_indexed_ws_f32", "geom_tri_distance_indexed_f32"), xyz1, faces.shape[0],
          (verts.shape[1], verts, faces.shape[0], faces), outputs, flags, use_workspace, order)
    return outputs


class TriDistanceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, tri1, tri2, tri3):
        dist, point, index = tri_distance(xyz1, tri1, tri2, tri3)
        ctx.mark_non_differentiable(dist, point, index)
        return dist, point, index

    @staticmethod
    def backward(ctx, *grads):
        return None, None, None, None


class TriDistance(torch.nn.Module):
    def forward(self, xyz1, tri1, tri2, tri3):
        return TriDistanceFunction.apply(xyz1, tri1, tri2, tri3)
