"""The projection-matrix pooling (the old driver's pooling(blocks, verts_pos, matrix), old_GEOMetrics/
utils.py:379-427) restated for the tests: features, the map gradient as P^T g and the position gradient in closed form, term by
term.  Pinned to the reference's own runs (tests/golden/pooling_matrix.npz) by test_matrix_pooling_host.py.

Everything is batched -- verts [B,V,3], proj [B,4,4], maps [B,C,d,d] -- and runs in the dtype of its arguments: float64 is the
yardstick, the SAME expressions in fp32 on the host are "the restatement's own fp32 run" the measured bars are derived from.
The projection is written element by element in the order geom_hip.h states (the reference's torch.mm leaves the order open):

    q_r = ((x*M[r][0] + y*M[r][1]) + z*M[r][2]) + M[r][3]   for r = 0, 1, 3        ys = (q0/q3 + 1)/2,  xs = 1 - (q1/q3 + 1)/2

Row 2 of the matrix is never read.  A NaN texel coordinate stands at texel 0 with zero weights on its axis (DESIGN.md section
5b: fminf(fmaxf(NaN, 0), hi) = 0); an infinite one is clamped like any far point.

The position gradient's term mass: d (xs, ys) / d vertex has TWO terms per entry,

    d ys / d p_j =  0.5 * (M[0][j]/q3 - q0*M[3][j]/q3^2),        d xs / d p_j = -0.5 * (M[1][j]/q3 - q1*M[3][j]/q3^2),

which an fp32 evaluation forms separately (the kernel: g0*M[0][j], g1*M[1][j] and g3*M[3][j] meet in one sum), so their
round-off does not shrink where they cancel: the mass and the floor carry |term 1| + |term 2| per entry (`J_abs`), the gradient
itself their signed sum."""
import numpy as np
import torch

EPS = float(np.finfo(np.float32).eps)
SHAPES = {"two_maps": ((3, 64), (2, 13)), "thin": ((6, 3, 5, 2), (5, 9, 40, 1))}
CAMERAS = ((35.0, 20.0, 1.2), (250.0, -30.0, 0.8), (60.0, 30.0, 1.0))      # family E: one camera per mesh of the union
G_SEED, G_SHARE = 7, 0.03                                                   # family G: E * (1 + 3 % * U(-1, 1)), row 2 = 1e30
# The bar for an entry of P (identity maps pooled) against float64, in eps * dim: MEASURED, not chosen -- 4 x the worst the
# restatement's own fp32 host run reaches on the kept vertices of the three meshes x {E, G} x P_DIMS (0.975, at 9 x 9, G on mesh
# 1), as POOL_P_ULPS of test_pooling_vertex_gradient_gpu.py was derived; test_matrix_pooling_host.py re-measures it.
P_DIMS = ((5, 9, 40, 1, 2, 13), (56, 28, 14, 7))        # the maps of the two ragged shapes; of the training shape (the 2 % cap: per group)
POOL_MATRIX_P_ULPS = 4 * 0.975


def meshes():
    """The three vertex sets of the ragged pooling tests: 2 x 101 vertices at three radii (the outer one partly off the image)
    and the first 70 of a jittered icosphere(2)."""
    from test_pooling_vertex_gradient_gpu import ragged_inputs, wide_inputs
    two = ragged_inputs()[0]
    return [two[0].contiguous(), two[1].contiguous(), wide_inputs()[0][1, :70].contiguous()]


def equivalent_matrices(cam_mat, cam_pos):
    """[B,4,4] float64: the matrices under which the matrix route projects as the camera route does with (cam_mat, cam_pos).
    With R = [0.57 * cam_mat | -cam_mat . cam_pos] ([3,4]: (X, Y, Z) = R . (x, y, z, 1)) and ys = (X/(-Z)*248 + 112)/223, xs =
    (Y/Z*248 + 112)/223:  q3 = 223 Z,  q0 = 223 Z (2 ys - 1) = -496 X + Z,  q1 = 223 Z (1 - 2 xs) = -496 Y - Z.  Row 2: zeros."""
    cam_mat, cam_pos = cam_mat.double(), cam_pos.double()
    R = torch.cat((0.57 * cam_mat, -(cam_mat * cam_pos[:, None, :]).sum(-1, keepdim=True)), dim=-1)          # [B,3,4]
    return torch.stack((-496.0 * R[:, 0] + R[:, 2], -496.0 * R[:, 1] - R[:, 2], torch.zeros_like(R[:, 0]), 223.0 * R[:, 2]), dim=1)


def family(name):
    """(the fp32 matrices [3,4,4] of family "E" or "G", the fp32 cameras (cam_mat, cam_pos) E is equivalent to)."""
    from oracle import ref_ops
    cam_mat, cam_pos = ref_ops.camera_info(torch.tensor(CAMERAS, dtype=torch.float64))
    E = equivalent_matrices(cam_mat, cam_pos)
    if name == "G":
        u = torch.rand(E.shape, generator=torch.Generator().manual_seed(G_SEED), dtype=torch.float64) * 2 - 1
        E = E * (1 + G_SHARE * u)
        E[:, 2] = 1e30
    return E.float(), (cam_mat.float(), cam_pos.float())


def maps_and_gradient(shape, nv, seed=32):
    """Seeded N(0, 1) maps [1,c,d,d] of one image and a cotangent [1,nv,sum c] (host generator: the same on every machine)."""
    chans, dims = SHAPES[shape]
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(1, c, d, d, generator=gen) for c, d in zip(chans, dims)], torch.randn(1, nv, sum(chans), generator=gen)


# ---------------------------------------------------------------- the restatement
def project(verts, proj):
    """(q0, q1, q3, xs, ys), [B,V] each, in the arguments' dtype and the header's order."""
    x, y, z = verts[..., 0], verts[..., 1], verts[..., 2]
    M = proj[:, None]                                                        # [B,1,4,4]
    q0, q1, q3 = (((x * M[..., r, 0] + y * M[..., r, 1]) + z * M[..., r, 2]) + M[..., r, 3] for r in (0, 1, 3))
    return q0, q1, q3, 1 - (q1 / q3 + 1) / 2, (q0 / q3 + 1) / 2


def texels(block, xs, ys):
    """ref_ops._pool_texels with the NaN rule: (rx, ry), (A, B, G, H), (c11, c12, c21, c22)."""
    b, c, dim = block.shape[0], block.shape[1], block.shape[-1]
    rx, ry = xs * dim, ys * dim
    cx = torch.where(torch.isnan(rx), torch.zeros_like(rx), torch.clamp(rx, 0, dim - 1))
    cy = torch.where(torch.isnan(ry), torch.zeros_like(ry), torch.clamp(ry, 0, dim - 1))
    x1, x2, y1, y2 = torch.floor(cx), torch.ceil(cx), torch.floor(cy), torch.ceil(cy)
    planes = block.reshape(b, c, dim * dim)

    def take(x, y):
        index = (x.long() * dim + y.long()).unsqueeze(1).expand(-1, c, -1)
        return torch.gather(planes, 2, index).transpose(1, 2)

    return (rx, ry), (x2 - cx, cx - x1, y2 - cy, cy - y1), (take(x1, y1), take(x1, y2), take(x2, y1), take(x2, y2))


def pool_features(blocks, verts, proj):
    """[B,V,sum C]; differentiable in the maps and the vertices by autograd."""
    _, _, _, xs, ys = project(verts, proj)
    out = []
    for block in blocks:
        _, (A, B, G, H), (c11, c12, c21, c22) = texels(block, xs, ys)
        A, B, G, H = (w.unsqueeze(-1) for w in (A, B, G, H))
        out.append(((A * c11 * G + H * c12 * A) + G * c21 * B) + B * c22 * H)
    return torch.cat(out, dim=-1)


def pool_operator(verts, proj, dim):
    """P [B,V,dim*dim]: the identity maps pooled (channel t = the one-hot map of texel t), in the arguments' dtype."""
    eye = torch.eye(dim * dim, dtype=verts.dtype).view(1, dim * dim, dim, dim).expand(verts.shape[0], -1, -1, -1)
    return pool_features([eye], verts, proj)


def pool_map_gradient(chans, dims, verts, proj, grad_out):
    """The map gradients as P^T g in float64: [(grad [B,c,d,d], mass [B,c,d,d] = sum |P||g|)] per map."""
    verts, proj, g = verts.double(), proj.double(), grad_out.double()
    out, col = [], 0
    for c, d in zip(chans, dims):
        P, gl = pool_operator(verts, proj, d), g[..., col:col + c]
        col += c
        out.append((torch.einsum("bvt,bvc->bct", P, gl).view(-1, c, d, d), torch.einsum("bvt,bvc->bct", P.abs(), gl.abs()).view(-1, c, d, d)))
    return out


def pool_vertex_gradient(blocks, verts, proj, grad_out):
    """d (sum grad_out * pool_features) / d verts in FLOAT64 from the closed form, term by term, in the shape
    oracle.ref_ops.pool_vertex_gradient returns: float64 numpy (grad [B,V,3], mass [B,V,3], floor [B,V,3], near [B,V]).  The
    per-map part (d f_c / d (x, y), the clamp as a select, one texel-coordinate ulp through every term, the distance to the
    nearest texel line) is that function's; the chain to the vertex is the matrix route's, with J_abs as the module says."""
    verts, proj, grad_out = (t.detach().double().cpu() for t in (verts, proj, grad_out))
    q0, q1, q3, xs, ys = project(verts, proj)
    M = proj[:, None]                                                        # [B,1,4,4]
    t1 = torch.stack((-0.5 * M[..., 1, :3] / q3[..., None], 0.5 * M[..., 0, :3] / q3[..., None]), dim=2)           # [B,V,2 (xs, ys),3]
    t2 = torch.stack((0.5 * (q1 / q3 ** 2)[..., None] * M[..., 3, :3], -0.5 * (q0 / q3 ** 2)[..., None] * M[..., 3, :3]), dim=2)
    J, J_abs = t1 + t2, t1.abs() + t2.abs()
    grad, mass, floor = (torch.zeros_like(verts) for _ in range(3))
    near = torch.full(verts.shape[:2], float("inf"), dtype=torch.float64)
    col = 0
    for block in blocks:
        c, dim = block.shape[1], block.shape[-1]
        (rx, ry), (A, B, G, H), (c11, c12, c21, c22) = texels(block.detach().double().cpu(), xs, ys)
        A, B, G, H = (w.unsqueeze(-1) for w in (A, B, G, H))
        g = grad_out[..., col:col + c]
        col += c
        inside = torch.stack(((rx >= 0) & (rx <= dim - 1), (ry >= 0) & (ry <= dim - 1)), dim=-1)                # [B,V,2]
        through = lambda t: torch.where(inside, t * dim, torch.zeros_like(t))
        terms = (torch.stack((-c11 * G, -H * c12, G * c21, c22 * H)), torch.stack((-A * c11, c12 * A, -c21 * B, B * c22)))
        d = through(torch.stack([(g * t.sum(0)).sum(-1) for t in terms], dim=-1))                              # [B,V,2]
        d_abs = through(torch.stack([(g.abs() * t.abs().sum(0)).sum(-1) for t in terms], dim=-1))
        ulp = through((EPS * dim * (g.abs() * (c11.abs() + c12.abs() + c21.abs() + c22.abs())).sum(-1)).unsqueeze(-1).expand(-1, -1, 2))
        # (a select again: an axis nothing came through contributes 0, not 0 * a non-finite J)
        chain = lambda s, j: torch.where((s != 0).unsqueeze(-1), s.unsqueeze(-1) * j, torch.zeros_like(j)).sum(2)
        grad += chain(d, J)
        mass += chain(d_abs, J_abs)
        floor += chain(ulp, J_abs)
        for r in (rx, ry):
            near = torch.minimum(near, (r - torch.clamp(torch.round(r), 0, dim - 1)).abs())
    return grad.numpy(), mass.numpy(), floor.numpy(), near.numpy()


def host_run(blocks, verts, proj, grad_out, dtype):
    """The restatement's own run in `dtype` on the host, by autograd: (features, verts.grad, [map gradients])."""
    v = verts.detach().to(dtype).requires_grad_(True)
    mm = [t.detach().to(dtype).requires_grad_(True) for t in blocks]
    feats = pool_features(mm, v, proj.to(dtype))
    got = torch.autograd.grad(feats, [v] + mm, grad_out.to(dtype))
    return feats.detach(), got[0], list(got[1:])


# ---------------------------------------------------------------- the bounds, shared by the host and the GPU tests
def kept_vertices(verts, proj, dims):
    """[B,V] bool: the vertices at least helpers.POOL_NEAR from every texel line of maps of sizes `dims` (float64); at most
    POOL_MAX_LEFT_OUT of them may sit closer (asserted)."""
    from helpers import POOL_MAX_LEFT_OUT, POOL_NEAR
    verts = torch.as_tensor(verts).detach().cpu()
    near = pool_vertex_gradient([torch.zeros(verts.shape[0], 1, d, d) for d in dims], verts, torch.as_tensor(proj).detach().cpu(),
                                torch.zeros(verts.shape[0], verts.shape[1], len(dims)))[3]
    keep = near >= POOL_NEAR
    assert (~keep).mean() <= POOL_MAX_LEFT_OUT, "%d of %d vertices within %g of a texel line of %s" % ((~keep).sum(), keep.size, POOL_NEAR, dims)
    return keep


def feature_bound(blocks, verts, proj, p_ulps=POOL_MATRIX_P_ULPS):
    """[B,V,sum C] float64, the bound for a feature of an fp32 evaluation: a feature is sum_t P[v,t] map[t], so |error| <= p_ulps
    eps dim (|c11| + |c12| + |c21| + |c22|) -- the bar for an entry of P through the four texels it can move -- + 8 eps sum |P||map|
    for the products and the sum."""
    _, _, _, xs, ys = project(verts.double().cpu(), proj.double().cpu())
    out = []
    for block in blocks:
        dim = block.shape[-1]
        _, (A, B, G, H), (c11, c12, c21, c22) = texels(block.detach().double().cpu().abs(), xs, ys)
        A, B, G, H = (w.unsqueeze(-1) for w in (A, B, G, H))
        out.append(p_ulps * EPS * dim * (c11 + c12 + c21 + c22) + 8 * EPS * (A * c11 * G + H * c12 * A + G * c21 * B + B * c22 * H))
    return torch.cat(out, -1)


def map_gradient_share(got, want, P, g, dim, keep, p_ulps=0.0):
    """The worst |got - want| / bound over a map gradient [c,d,d] of ONE mesh, bound = 8 eps sum |P||g| + p_ulps eps dim sum |g| over
    the vertices that reach the texel.  P [V,d*d]: float64, the weights `want` was formed with; p_ulps > 0 when `got` formed its
    OWN fp32 weights (the bar for an entry of P).  keep [V]: the texels a left-out vertex reaches, and their neighbours (in fp32
    it may reach the next one), are not compared when p_ulps > 0."""
    P, g = P.double(), g.double()
    bound = 8 * EPS * torch.einsum("vt,vc->ct", P.abs(), g.abs()) + p_ulps * EPS * dim * torch.einsum("vt,vc->ct", (P != 0).double(), g.abs()) + 1e-30
    flat = lambda t: torch.as_tensor(t).detach().cpu().double().reshape(-1, dim * dim)
    err = (flat(got) - flat(want)).abs()
    skip = torch.zeros(dim * dim, dtype=torch.bool)
    if p_ulps > 0:
        skip = P[~torch.as_tensor(keep)].abs().sum(0) > 0
        if dim > 1:
            skip = (torch.nn.functional.max_pool2d(skip.view(1, 1, dim, dim).double(), 3, 1, 1) > 0).view(-1)
    share = (err / bound)[:, ~skip]
    return float(share.max()) if share.numel() else 0.0


def vertex_gradient_close(got, blocks, verts, proj, grad_out, what, against=None):
    """helpers.pool_vertex_gradient_close for the matrix route: `got` [B,V,3] against pool_vertex_gradient element by element with
    rows_close(POOL_ROW_RTOL of the term mass + POOL_FLOOR_ULPS texel-coordinate ulps through every term) on the vertices at
    least POOL_NEAR from every texel line (at most POOL_MAX_LEFT_OUT of them may sit closer), and exactly zero rows where the
    float64 row is exactly zero.  against [B,V,3]: another evaluation to hold `got` to under the same bounds (the float64 terms
    still give the mass, the floor and the zero rows).  Returns the same record."""
    from helpers import POOL_FLOOR_ULPS, POOL_MAX_LEFT_OUT, POOL_NEAR, POOL_ROW_RTOL, rows_close
    cpu = lambda t: torch.as_tensor(t).detach().cpu()
    grad, mass, floor, near = pool_vertex_gradient([cpu(m) for m in blocks], cpu(verts), cpu(proj), cpu(grad_out))
    keep = near >= POOL_NEAR
    assert (~keep).mean() <= POOL_MAX_LEFT_OUT, "%s: %d of %d vertices within %g of a texel line" % (what, (~keep).sum(), keep.size, POOL_NEAR)
    got = cpu(got).numpy()
    zero = keep & (grad == 0).all(-1)
    assert (got[zero] == 0).all(), "%s: a vertex the clamp holds on both axes has a gradient" % what
    live = keep & ~zero
    exact = grad if against is None else np.asarray(cpu(against).numpy(), np.float64)
    worst = rows_close(got[live], exact[live], mass[live], POOL_ROW_RTOL, what, floor=floor[live], floor_ulps=POOL_FLOOR_ULPS)
    return {"keep": keep, "zero_rows": int((grad == 0).all(-1).sum()), "zero_checked": int(zero.sum()), "live_rows": int(live.sum()),
            "worst": worst}


def weights_error(P, verts, proj, dim, keep):
    """P [B,V,dim*dim] of an fp32 evaluation against the float64 operator on the kept vertices, in eps * dim; an entry that is
    zero on one side only is a failure whatever its size."""
    exact = pool_operator(verts.double().cpu(), proj.double().cpu(), dim)[torch.as_tensor(keep)]
    P = torch.as_tensor(P).detach().double().cpu()[torch.as_tensor(keep)]
    assert bool(((P == 0) == (exact == 0)).all()), "%d x %d: a weight is zero on one side only" % (dim, dim)
    return float((P - exact).abs().max()) / (EPS * dim)
