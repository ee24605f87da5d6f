"""CPU restatement (torch, any float dtype) of the differentiable python stages of the
GEOMetrics hot path -- TEST INFRASTRUCTURE ONLY, never imported by geometrics_amd.

Each function states the reference lines it follows.  They are pinned against fixtures
emitted by the imported reference itself (tests/golden/make_golden.py ->
tests/test_oracle_pin.py) and then serve as the checker at sizes where no fixture is
stored (2562-vertex meshes), with the arg-min stages taken from the C oracle.
"""
import numpy as np
import torch

import oracle


def sample_points(verts, faces, choices, u, v):
    """utils.py:615-631: gather the three corners of each chosen face, then
    ((1-u)*x + (u*(1-v))*y) + (u*v)*z.  choices [B,S] face ids; u is already sqrt'ed."""
    b = verts.shape[0]
    sel = faces[choices.reshape(-1)].view(b, -1, 3)                      # [B,S,3] vertex ids
    x, y, z = (torch.gather(verts, 1, sel[..., k:k + 1].expand(-1, -1, 3)) for k in range(3))
    u = u.unsqueeze(-1)
    v = v.unsqueeze(-1)
    return (1 - u) * x + (u * (1 - v)) * y + u * v * z


def face_areas(verts, faces):
    """utils.py:596-602 (un-normalised)."""
    x = verts[:, faces[:, 0]] - verts[:, faces[:, 1]]
    y = verts[:, faces[:, 1]] - verts[:, faces[:, 2]]
    a = (x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1]) ** 2
    b = (x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2]) ** 2
    c = (x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]) ** 2
    return torch.sqrt(a + b + c) / 2


def _nn(gt, pred, flags=0):
    """flags = oracle.FLAG_REF_TAIL_TRUNC: the shipped CUDA kernel's tile structure (chamfer_distance.cu:6-55) instead of the
    full sequential scan."""
    _, idx_p, _, idx_g = oracle.chamfer_nn(gt.detach().float().numpy(), pred.detach().float().numpy(), flags)
    return torch.from_numpy(idx_p).long(), torch.from_numpy(idx_g).long()


def _f1(pred_counters, gt_counters, pred, gt, num):
    """utils.py:424-436 / 489-500."""
    to_pred = torch.sqrt(((.57 * pred_counters - .57 * gt) ** 2).sum(-1))
    to_gt = torch.sqrt(((.57 * gt_counters - .57 * pred) ** 2).sum(-1))
    score = 0.0
    for i in range(to_pred.shape[0]):
        recall = float((to_pred[i] <= 1e-2).sum()) / float(num)
        precision = float((to_gt[i] <= 1e-2).sum()) / float(num)
        score += 2 * (precision * recall) / (precision + recall + 1e-8)
    return score / to_pred.shape[0]


def point_to_point(verts, faces, gt, choices, u, v, f1=False, nn_flags=0):
    """utils.py:393-438 with the draws replayed."""
    pred = sample_points(verts, faces, choices, u, v)
    idx_p, idx_g = _nn(gt, pred, nn_flags)
    pred_counters = torch.gather(pred, 1, idx_p.unsqueeze(-1).expand(-1, -1, 3))
    gt_counters = torch.gather(gt, 1, idx_g.unsqueeze(-1).expand(-1, -1, 3))
    dist_1 = ((gt_counters - pred) ** 2).sum(-1).mean()
    dist_2 = ((pred_counters - gt) ** 2).sum(-1).mean()
    loss = (dist_1 + dist_2) * 3000
    return (loss, _f1(pred_counters, gt_counters, pred, gt, choices.shape[1])) if f1 else loss


def closest_point(p, a, b, c, option):
    """utils.py:506-548: candidate selected by option (1,2,3 corners; 4,5,6 edge points with the
    CORRECT deltas; 0 plane projection).  All [N,3]; option [N]."""
    def proj(org, delta):
        return ((p - org) * delta).sum(-1) / (delta ** 2).sum(-1)

    uab, ubc, uca = proj(a, b - a), proj(b, c - b), proj(c, a - c)
    n = torch.cross(a - b, a - c, dim=-1)
    n = n / torch.sqrt((n ** 2).sum(-1)).unsqueeze(-1)
    plane = p - ((p - a) * n).sum(-1, keepdim=True) * n
    cands = [plane, a, b, c, a + uab.unsqueeze(-1) * (b - a), b + ubc.unsqueeze(-1) * (c - b),
             c + uca.unsqueeze(-1) * (a - c)]
    out = torch.zeros_like(p)
    for code, cand in enumerate(cands):
        out = torch.where((option == code).unsqueeze(-1), cand, out)
    return out


def point_to_line(p, a, b, c, option):
    """utils.py:549: mean squared distance to the selected candidate."""
    return ((closest_point(p, a, b, c, option) - p) ** 2).sum(-1).mean()


def point_to_surface(verts, faces, gt, choices, u, v, f1=False, tri_flags=0, nn_flags=0):
    """utils.py:441-502 with the draws replayed; the tri scan is the C oracle."""
    pred = sample_points(verts, faces, choices, u, v)
    idx_p, idx_g = _nn(gt, pred, nn_flags)
    pred_counters = torch.gather(pred, 1, idx_p.unsqueeze(-1).expand(-1, -1, 3))
    gt_counters = torch.gather(gt, 1, idx_g.unsqueeze(-1).expand(-1, -1, 3))
    dist_1 = ((gt_counters - pred) ** 2).sum(-1).mean()
    _, opt, idx = oracle.tri_scan_indexed(gt.detach().float().numpy(), verts.detach().float().numpy(),
                                          faces.numpy(), tri_flags)
    idx = torch.from_numpy(idx).long()
    corners = [torch.gather(verts[:, faces[:, k]], 1, idx.unsqueeze(-1).expand(-1, -1, 3)).reshape(-1, 3)
               for k in range(3)]
    dist_2 = point_to_line(gt.reshape(-1, 3), *corners, torch.from_numpy(opt).reshape(-1))
    loss = (dist_1 + dist_2) * 3000
    return (loss, _f1(pred_counters, gt_counters, pred, gt, choices.shape[1])) if f1 else loss


def calc_adj(faces):
    """utils.py:115-131."""
    n = int(faces.max()) + 1
    adj = torch.eye(n)
    for i, j in ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)):
        adj[faces[:, i], faces[:, j]] = 1
    return adj


def normalize_adj(mx):
    """utils.py:96-101."""
    r_inv = 1.0 / mx.sum(1)
    r_inv[r_inv != r_inv] = 0.0
    return torch.diag(r_inv) @ mx


def dense_aggregate(adj, support):
    """adj @ support: the reference's product (layers.py:38).  0 * NaN is NaN there: one non-finite value of `support` reaches
    every row of its column."""
    return adj @ support


def sparse_aggregate(adj, support):
    """The same sum over the NON-ZEROS of `adj` [V,V] alone -- what a CSR row or a neighbour table holds, and so what the
    kernels add up: a non-finite value of `support` [...,V,k] reaches the rows that have its vertex as a neighbour and no
    other.  Differentiable; on finite operands equal to dense_aggregate up to the round-off of the rows' sums."""
    rows, cols = torch.nonzero(adj, as_tuple=True)
    val = adj[rows, cols].to(support.dtype)
    out = torch.zeros_like(support)
    return out.index_add(-2, rows, val[:, None] * support[..., cols, :])


def zero_n_layer(x, adj, weight, bias, split, activation, aggregate=dense_aggregate):
    """layers.py:34-41 / 107-116 / 143-152: support = x W; first C//split columns multiplied by
    the dense adjacency (aggregate: dense_aggregate or sparse_aggregate); concat; + bias; activation."""
    if weight.dim() == 3:
        weight = weight[0]
    support = x @ weight
    k = support.shape[-1] // split
    out = torch.cat((aggregate(adj, support[..., :k]), support[..., k:]), dim=-1)
    if bias is not None:
        out = out + bias
    return activation(out)


def gcn_max(x, adj, weight, bias, activation, batched):
    """layers.py:61-79 (max of the activation) / 175-189 (max of the PRE-activation)."""
    v = zero_n_layer(x, adj, weight, bias, 10, lambda t: t)
    return torch.max(v, dim=1)[0] if batched else torch.max(activation(v), dim=0)[0]


def as_np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def lap_info(positions, adj_orig):
    """utils.py:654-662: dense neighbour sum minus self, divided by (degree), subtracted from positions."""
    neighbour_sum = torch.matmul(adj_orig, positions) - positions
    scaler = (1.0 / (adj_orig.sum(1) - 1)).view(-1, 1)
    return positions - neighbour_sum * scaler


def calc_edge(verts, faces):
    """utils.py:636-651."""
    p1, p2, p3 = (verts[:, faces[:, k]] for k in range(3))
    return (((p2 - p1) ** 2).sum(-1).mean() + ((p3 - p1) ** 2).sum(-1).mean() + ((p2 - p3) ** 2).sum(-1).mean()) / 3.0


ENCODER_LAYERS = ("h1", "h21", "h22", "h23", "h24", "h3", "h4", "h41", "h5", "h6", "h7", "h8", "h81", "h9", "h10", "h11")


def mesh_encoder(params, positions, adj):
    """models.py:324-348 for one mesh: 16 ELU 0N-GCN layers (split 10), then GCNMax (layers.py:61-79).
    params: {name: tensor} with the reference's state_dict keys."""
    elu = torch.nn.functional.elu
    x = positions
    for name in ENCODER_LAYERS:
        x = zero_n_layer(x, adj, params[name + ".weight"], params[name + ".bias"], 10, elu)
    return gcn_max(x, adj, params["reduce.weight_Ws.0"], params["reduce.weight_Bs.0"], elu, batched=False)


def segment_max(x, sizes):
    """Per-mesh column max of rows concatenated along dim 0 (layers.py:78 applied mesh by mesh)."""
    return torch.stack([part.max(dim=0)[0] for part in torch.split(x, list(sizes), dim=0)])


# ---- image-feature pooling (utils.py:286-389) -------------------------------------------------------------------------------
POOL_SCALE, POOL_FOCAL, POOL_HALF, POOL_NORM = 0.57, 248.0, 224.0 / 2.0, 223.0


def camera_info(param):
    """utils.py:286-313: rotation rows [B,3,3] (the camera's x, y, z axes, normalised) and position [B,3] from
    (azimuth deg, elevation deg, distance); the `%` is torch.remainder."""
    theta = (np.pi * param[:, 0] / 180.0) % 360.0
    phi = (np.pi * param[:, 1] / 180.0) % 360.0
    flat = param[:, 2] * torch.cos(phi)
    pos = torch.stack((flat * torch.cos(theta), param[:, 2] * torch.sin(phi), flat * torch.sin(theta)), dim=1)
    up = torch.zeros_like(pos)
    up[:, 1] = 1.0
    x = torch.cross(up, pos, dim=1)
    y = torch.cross(pos, x, dim=1)
    return torch.stack([a / torch.sqrt((a ** 2).sum(1, keepdim=True)) for a in (x, y, pos)], dim=1), pos


def _pool_project(verts, cam_mat, cam_pos):
    """utils.py:321-333: camera-space (X, Y, Z) [B,V] each and the image fractions (xs, ys) [B,V] of every vertex."""
    a = verts * POOL_SCALE - cam_pos.unsqueeze(1)
    X, Y, Z = ((a[..., 0] * cam_mat[:, None, r, 0] + a[..., 1] * cam_mat[:, None, r, 1]) + a[..., 2] * cam_mat[:, None, r, 2]
               for r in range(3))
    xs = ((-Y) / (-Z) * POOL_FOCAL + POOL_HALF) / POOL_NORM
    ys = (X / (-Z) * POOL_FOCAL + POOL_HALF) / POOL_NORM
    return X, Y, Z, xs, ys


def _pool_texels(block, xs, ys):
    """utils.py:339-371 for one map [B,C,d,d]: the unclamped texel coordinates (rx, ry), the weights A = x2 - x, B = x - x1,
    G = y2 - y, H = y - y1 of the CLAMPED coordinate ([B,V] each; all zero where it is integral) and the four texels' values
    c11, c12, c21, c22 [B,V,C] (first index x1 / x2, second y1 / y2)."""
    b, c, dim = block.shape[0], block.shape[1], block.shape[-1]
    rx, ry = xs * dim, ys * dim
    cx, cy = torch.clamp(rx, 0, dim - 1), torch.clamp(ry, 0, dim - 1)
    x1, x2, y1, y2 = torch.floor(cx), torch.ceil(cx), torch.floor(cy), torch.ceil(cy)
    planes = block.reshape(b, c, dim * dim)

    def take(x, y):
        index = (x.long() * dim + y.long()).unsqueeze(1).expand(-1, c, -1)
        return torch.gather(planes, 2, index).transpose(1, 2)

    return (rx, ry), (x2 - cx, cx - x1, y2 - cy, cy - y1), (take(x1, y1), take(x1, y2), take(x2, y1), take(x2, y2))


def pool_features(blocks, verts, cam_mat, cam_pos):
    """utils.py:316-389 with the camera of batch_camera_info handed in: [B,V,sum C] features of the maps `blocks` (each
    [B,C,d,d]) at the pixels the vertices [B,V,3] project to.  Any float dtype (of all arguments alike); differentiable
    in the maps and the vertices by autograd."""
    _, _, _, xs, ys = _pool_project(verts, cam_mat, cam_pos)
    out = []
    for block in blocks:
        _, (A, B, G, H), (c11, c12, c21, c22) = _pool_texels(block, xs, ys)
        A, B, G, H = (w.unsqueeze(-1) for w in (A, B, G, H))
        out.append(((A * c11 * G + H * c12 * A) + G * c21 * B) + B * c22 * H)
    return torch.cat(out, dim=-1)


def pool_vertex_gradient(blocks, verts, cam_mat, cam_pos, grad_out):
    """d (sum grad_out * pool_features) / d verts in FLOAT64 from the closed form, TERM BY TERM -- one term per (vertex, map,
    channel).  With f_c = A c11 G + H c12 A + G c21 B + B c22 H and floor / ceil piecewise constant,
        d f_c / d x = (-c11 G - H c12) + (G c21 + c22 H),     d f_c / d y = (-A c11 + c12 A) + (-c21 B + B c22)
    per texel; a texel coordinate is xs * dim, the clamp to [0, dim - 1] passes the gradient only inside (bounds included; a select), and
    J = d (xs, ys) / d vertex [B,V,2,3] chains through the perspective divide, the camera matrix and the 0.57.  Returns float64
    numpy arrays in the sense of helpers.fp64_surface_gradient / helpers.rows_close:
      grad  [B,V,3]  sum_c g_c * d f_c / d (x, y) * dim * [inside the clamp] * J;
      mass  [B,V,3]  the same sum with every factor's absolute value, the four texel terms of d f_c taken separately: the scale an
                     fp32 evaluation's round-off is proportional to, whatever cancels;
      floor [B,V,3]  one fp32 ulp of a texel coordinate (eps * dim) through every term: the weights are differences of the fp32
                     xs * dim and a whole number, so their ABSOLUTE rounding does not shrink with the weight --
                     eps * dim^2 * sum_c |g_c| (|c11| + |c12| + |c21| + |c22|) |J| on the axes the clamp lets through;
      near  [B,V]    the smallest distance, over the maps and both axes, of the unclamped texel coordinate to the nearest texel
                     line 0 ... dim - 1: the gradient is discontinuous across a line, a comparison with an fp32 evaluation
                     leaves out the vertices that sit on one."""
    eps = float(np.finfo(np.float32).eps)
    verts, cam_mat, cam_pos, grad_out = (t.detach().double().cpu() for t in (verts, cam_mat, cam_pos, grad_out))
    X, Y, Z, xs, ys = _pool_project(verts, cam_mat, cam_pos)
    # xs = (Y / Z * F + 112) / 223,  ys = (-X / Z * F + 112) / 223;  d (X, Y, Z) / d vertex = 0.57 * the camera's rows
    k = POOL_FOCAL / POOL_NORM
    rows = POOL_SCALE * cam_mat[:, None]                                                       # [B,1,3 (X,Y,Z),3]
    J = torch.stack(((k / Z).unsqueeze(-1) * rows[:, :, 1] + (-k * Y / Z ** 2).unsqueeze(-1) * rows[:, :, 2],
                     (-k / Z).unsqueeze(-1) * rows[:, :, 0] + (k * X / Z ** 2).unsqueeze(-1) * rows[:, :, 2]), dim=2)
    grad, mass, floor = (torch.zeros_like(verts) for _ in range(3))
    near = torch.full(verts.shape[:2], float("inf"), dtype=torch.float64)
    col = 0
    for block in blocks:
        c, dim = block.shape[1], block.shape[-1]
        (rx, ry), (A, B, G, H), (c11, c12, c21, c22) = _pool_texels(block.detach().double().cpu(), xs, ys)
        A, B, G, H = (w.unsqueeze(-1) for w in (A, B, G, H))
        g = grad_out[..., col:col + c]
        col += c
        inside = torch.stack(((rx >= 0) & (rx <= dim - 1), (ry >= 0) & (ry <= dim - 1)), dim=-1)                # [B,V,2]
        # (the clamp's backward is a SELECT, as torch's: a non-finite term behind a clamp that holds is 0, not 0 * NaN)
        through = lambda t: torch.where(inside, t * dim, torch.zeros_like(t))
        terms = (torch.stack((-c11 * G, -H * c12, G * c21, c22 * H)), torch.stack((-A * c11, c12 * A, -c21 * B, B * c22)))
        d = through(torch.stack([(g * t.sum(0)).sum(-1) for t in terms], dim=-1))                              # [B,V,2]
        d_abs = through(torch.stack([(g.abs() * t.abs().sum(0)).sum(-1) for t in terms], dim=-1))
        ulp = through((eps * dim * (g.abs() * (c11.abs() + c12.abs() + c21.abs() + c22.abs())).sum(-1)).unsqueeze(-1).expand(-1, -1, 2))
        grad += (d.unsqueeze(-1) * J).sum(2)
        mass += (d_abs.unsqueeze(-1) * J.abs()).sum(2)
        floor += (ulp.unsqueeze(-1) * J.abs()).sum(2)
        for r in (rx, ry):
            near = torch.minimum(near, (r - torch.clamp(torch.round(r), 0, dim - 1)).abs())
    return grad.numpy(), mass.numpy(), floor.numpy(), near.numpy()
