"""Shared by tests/test_nonfinite_ops_host.py and tests/test_nonfinite_ops_gpu.py: the host restatements of what the sampler, the
optimiser and the pooling do with a NaN or an Inf, each with the planted fault its test is shown to catch.
Everything here runs on the host (numpy / torch CPU)."""
import numpy as np
import torch

import draw_helpers as dh

NAN, INF = float("nan"), float("inf")
VALUES = {"nan": NAN, "+inf": INF, "-inf": -INF}


# ---- the face sampler ------------------------------------------------------------------------------------------------------
def faces_of_vertex(faces, v):
    return np.flatnonzero((faces == v).any(axis=1))


def sampler_plants(faces):
    """{name: vertex}: a vertex of face 0 (every face behind it was lost to an unconditional running sum), a vertex one of whose
    faces shares its THREAD with a face that does not touch it (two faces per thread: the thread's local sum holds a NaN area in
    front of or behind a good one; one face per thread: any face of the middle), and a vertex of the last face."""
    nf = faces.shape[0]
    per = (nf + dh.THREADS - 1) // dh.THREADS
    boundary = None
    for f in range(nf // 2, nf):
        for v in faces[f]:
            touched = set(faces_of_vertex(faces, v).tolist())
            mates = range((f // per) * per, min((f // per + 1) * per, nf))
            if per == 1 or any(m not in touched for m in mates):
                boundary = int(v)
                break
        if boundary is not None:
            break
    return {"low": int(faces[0, 0]), "boundary": boundary, "last": int(faces[nf - 1, 2])}


def planted_vertex(verts, v, value, axis=1):
    out = np.array(verts, dtype=np.float32, copy=True)
    out[..., v, axis] = value
    return out


def remaining_areas_f64(verts, faces):
    """float64 areas with every face whose fp32 area is not `> 0` (NaN, zero) weighing nothing: the distribution the rule leaves."""
    with np.errstate(invalid="ignore", over="ignore"):
        a32 = dh.face_areas_f32(verts, faces)
        a64 = dh.face_areas_f64(np.where(np.isfinite(verts), verts, 0).astype(np.float32), faces)
    return np.where(a32 > 0, a64, 0.0)


def unconditional_table(areas):
    """THE PLANTED FAULT: the table of a running sum that adds every area (`run += area`), as the kernel did -- the NaN area
    poisons its thread's sum and the offset of every later thread, fmax passes over all of them."""
    areas = np.asarray(areas, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return dh.table(areas, sums=dh.scanned_sums_f32(areas))


def same_floats(a, b):
    """Bit for bit where finite or Inf; NaN where the other is NaN (sign and payload of a NaN are not pinned)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


# ---- Adam ------------------------------------------------------------------------------------------------------------------
ADAM_LR, ADAM_BETAS, ADAM_EPS = 1e-2, (0.9, 0.999), 1e-8
ADAM_RTOL, ADAM_ATOL = 2e-5, 2e-6             # test_table_route_tracks_torch_adam's (torch.allclose)


def adam_rule64(params, grads_per_step, skip_nonfinite=False):
    """The written rule (csrc/adam_math.h, torch.optim.Adam's documentation) in float64, step by step:
        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    -> [(p, m, v) lists of float64 numpy arrays after step 1, 2, ...].  skip_nonfinite: THE PLANTED FAULT -- an update that
    leaves an element alone whose gradient is not finite."""
    b1, b2 = ADAM_BETAS
    p = [np.asarray(t, np.float64).copy() for t in params]
    m, v = [np.zeros_like(t) for t in p], [np.zeros_like(t) for t in p]
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for t, grads in enumerate(grads_per_step, 1):
            for i, g in enumerate(grads):
                g = np.asarray(g, np.float64)
                mi = b1 * m[i] + (1 - b1) * g
                vi = b2 * v[i] + (1 - b2) * g * g
                pi = p[i] - ADAM_LR / (1 - b1 ** t) * (mi / (np.sqrt(vi) / np.sqrt(1 - b2 ** t) + ADAM_EPS))
                if skip_nonfinite:
                    ok = np.isfinite(g)
                    mi, vi, pi = np.where(ok, mi, m[i]), np.where(ok, vi, v[i]), np.where(ok, pi, p[i])
                m[i], v[i], p[i] = mi, vi, pi
            out.append(([a.copy() for a in p], [a.copy() for a in m], [a.copy() for a in v]))
    return out


def adam_torch64(params, grads_per_step):
    """torch.optim.Adam on the host in float64, same hyperparameters -> the same structure as adam_rule64."""
    ps = [torch.as_tensor(np.asarray(t, np.float64)).clone().requires_grad_(True) for t in params]
    opt = torch.optim.Adam(ps, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS)
    out = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = torch.as_tensor(np.asarray(g, np.float64)).clone()
        opt.step()
        out.append(([p.detach().numpy().copy() for p in ps], [opt.state[p]["exp_avg"].numpy().copy() for p in ps],
                    [opt.state[p]["exp_avg_sq"].numpy().copy() for p in ps]))
    return out


def adam_mass(want):
    """The mass under which helpers.rows_close(rtol = ADAM_RTOL) is torch.allclose(rtol = ADAM_RTOL, atol = ADAM_ATOL)."""
    return np.where(np.isfinite(want), np.abs(want), 0.0) + ADAM_ATOL / ADAM_RTOL


# ---- the pooling -----------------------------------------------------------------------------------------------------------
def pool_weights64(verts, cam_mat, cam_pos, dim):
    """The pooling operator of one map size as the RULE states it, float64: (index [B,V,4] int64, weight [B,V,4]) -- the four
    corners 11, 12, 21, 22 of every vertex with the reference's weights G A, A H, B G, H B (oracle/ref_ops.py).  A vertex whose
    projection is NaN stands at texel 0 with four zero weights (fminf(fmaxf(NaN, 0), hi) = 0)."""
    from oracle import ref_ops
    _, _, _, xs, ys = ref_ops._pool_project(verts.double(), cam_mat.double(), cam_pos.double())
    rx, ry = xs * dim, ys * dim
    cx = torch.where(torch.isnan(rx), torch.zeros_like(rx), torch.clamp(rx, 0, dim - 1))
    cy = torch.where(torch.isnan(ry), torch.zeros_like(ry), torch.clamp(ry, 0, dim - 1))
    x1, x2, y1, y2 = torch.floor(cx), torch.ceil(cx), torch.floor(cy), torch.ceil(cy)
    A, B, G, H = x2 - cx, cx - x1, y2 - cy, cy - y1
    index = torch.stack([(a.long() * dim + b.long()) for a, b in ((x1, y1), (x1, y2), (x2, y1), (x2, y2))], dim=-1)
    weight = torch.stack((G * A, A * H, B * G, H * B), dim=-1)
    return index, weight, torch.isnan(rx) | torch.isnan(ry)


def pool_forward64(block, index, weight):
    """feats [B,V,C] = sum over the four corners of weight * texel, every product FORMED (0 * NaN is NaN, as in the reference's
    expression and in the kernel's forward)."""
    b, c, dim = block.shape[0], block.shape[1], block.shape[-1]
    planes = block.double().reshape(b, c, dim * dim)
    out = torch.zeros(b, index.shape[1], c, dtype=torch.float64)
    for k in range(4):
        tex = torch.gather(planes, 2, index[..., k].unsqueeze(1).expand(-1, c, -1)).transpose(1, 2)       # [B,V,C]
        out = out + weight[..., k].unsqueeze(-1) * tex
    return out


def pool_map_gradient64(grad_out, index, weight, dim, stored_only=True):
    """d loss / d map [B,C,dim,dim] in float64 and its mass: the sum over the STORED corners -- those of non-zero weight, what
    `corners()` of csrc/pooling.hip lists -- of weight * grad_out[b, v, c].  stored_only=False: THE PLANTED FAULT, the
    "multiply by the zero weight" form (autograd's: 0 * NaN poisons the texel of every zero-weight corner)."""
    g = grad_out.double()
    b, nv, c = g.shape
    grad = torch.zeros(b, c, dim * dim, dtype=torch.float64)
    mass = torch.zeros_like(grad)
    fin = torch.where(torch.isfinite(g), g, torch.zeros_like(g)).abs()
    for k in range(4):
        w = weight[..., k]
        keep = (w != 0) if stored_only else torch.ones_like(w, dtype=torch.bool)
        for m in range(b):
            rows = torch.nonzero(keep[m]).flatten()
            if rows.numel() == 0:
                continue
            term = w[m, rows].unsqueeze(0) * g[m, rows].t()                                # [C, rows]
            grad[m].index_add_(1, index[m, rows, k], term)
            mass[m].index_add_(1, index[m, rows, k], w[m, rows].abs().unsqueeze(0) * fin[m, rows].t())
    return grad.view(b, c, dim, dim), mass.view(b, c, dim, dim)
