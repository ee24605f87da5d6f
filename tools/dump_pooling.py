"""Every launch of csrc/pooling.hip, once, on seeded host-generated inputs, through the C ABI; each output as <name>.npy.

    python tools/dump_pooling.py OUTDIR [MAPGRAD_DIR]        (MAPGRAD_DIR: default OUTDIR + "_mapgrads")

Run from two checkouts on the same GPU, the two OUTDIRs must compare byte for byte (cmp, or `diff -r`): the check behind a
change that may move no result bit (profiles/pooling_refactor.txt).  OUTDIR holds the features (the whole wide buffer where the
launch also places fronts), verts.grad, the texel lists' offsets and the lists themselves sorted per texel by vertex (their order
inside a texel follows an atomic cursor), the cameras of batch_camera_info, and calls.txt, the entry points every case took.
The map gradients are sums in list order -- not bit-stable from run to run -- and go to MAPGRAD_DIR, each beside the per-element
bound of the float64 tests, 8 eps * sum |P||g| (tests/test_ops_parity_gpu.py: _pooling_against_float64): two dumps are compared
element by element as a share of that bound."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from geometrics_amd import _lib, meshgen, utils  # noqa: E402

OUT = GRADS = None
CALLS = []
EPS = float(np.finfo(np.float32).eps)


def save(name, t, where=None):
    t = t.detach().contiguous().cpu()
    np.save(os.path.join(where or OUT, name + ".npy"), t.view(torch.int32).numpy() if t.dtype == torch.float32 else t.numpy())


def carray(kind, values):
    return (kind * len(values))(*values)


def ragged_inputs():
    V, _ = meshgen.icosphere(1)
    V = np.concatenate([V, 0.5 * V, 2.5 * V], 0)[:101]      # the outer radius leaves the image for some cameras
    return meshgen.jittered_batch(V, 2), [[35.0, 20.0, 1.2], [250.0, -30.0, 0.8]]


def training_inputs():
    V, _ = meshgen.icosphere(2)
    V = np.concatenate([V, 0.6 * V, 0.3 * V], 0)[:482]
    return meshgen.jittered_batch(V, 3), [[35.0, 20.0, 1.2], [200.0, -10.0, 1.0], [310.0, 45.0, 1.4]]


def wide_inputs():
    V, _ = meshgen.icosphere(2)
    return meshgen.jittered_batch(V, 2), [[35.0, 20.0, 1.2], [60.0, 30.0, 1.0]]


def pooled(verts, cams, maps, out, ld, fronts=(), buf=None):
    """geom_pool_features_fwd_ld_f32, or _fronts_f32 when there are fronts [(tensor, first column)]."""
    b, nv = verts.shape[:2]
    n = len(maps)
    args = [b, nv, verts.data_ptr(), cams[0].data_ptr(), cams[1].data_ptr(), n, carray(ctypes.c_void_p, [t.data_ptr() for t in maps]),
            carray(ctypes.c_int, [t.shape[1] for t in maps]), carray(ctypes.c_int, [t.shape[2] for t in maps]), out.data_ptr(), ld]
    if not fronts:
        return _lib.call("geom_pool_features_fwd_ld_f32", *args)
    _lib.call("geom_pool_features_fwd_fronts_f32", *args, len(fronts), carray(ctypes.c_void_p, [t.data_ptr() for t, _ in fronts]),
              carray(ctypes.c_int, [t.shape[2] for t, _ in fronts]), carray(ctypes.c_int, [c for _, c in fronts]), buf.data_ptr())


def sorted_lists(ws, b, nv, dims):
    """offsets [b, sum(dim^2 + 1)] and the (vertex, weight bits) entries [b, levels, 4 nv] of the workspace (layout:
    include/geom_hip.h), every texel's list sorted by vertex; the slots past a map's last entry are zeroed."""
    per_mesh, n = sum(d * d + 1 for d in dims), len(dims)
    ent0, ent = (b * per_mesh * 4 + 15) // 16 * 16 // 4, b * n * 4 * nv
    offsets = ws[:b * per_mesh].reshape(b, per_mesh)
    ent_v = ws[ent0:ent0 + ent].reshape(b, n, 4 * nv).copy()
    ent_w = ws[ent0 + ent:ent0 + 2 * ent].reshape(b, n, 4 * nv).copy()
    for mesh in range(b):
        lo = 0
        for l, d in enumerate(dims):
            offs = offsets[mesh, lo:lo + d * d + 1].astype(np.int64)
            total = int(offs[-1])
            texel = np.searchsorted(offs, np.arange(total), side="right") - 1
            order = np.argsort(texel * nv + ent_v[mesh, l, :total], kind="stable")
            ent_v[mesh, l, :total], ent_w[mesh, l, :total] = ent_v[mesh, l, :total][order], ent_w[mesh, l, :total][order]
            ent_v[mesh, l, total:], ent_w[mesh, l, total:] = 0, 0
            lo += d * d + 1
    return offsets, ent_v, ent_w


def case(name, inputs, chans, dims, headroom=0, fronts=False, maps_grad=True):
    torch.cuda.synchronize()
    CALLS.append("== " + name)
    V, info = inputs
    gen = torch.Generator(device="cpu").manual_seed(len(name) + 31 * headroom + sum(chans))
    verts = torch.from_numpy(np.ascontiguousarray(V)).cuda()
    cams = utils.batch_camera_info(torch.tensor(info).cuda())
    b, nv = verts.shape[:2]
    maps = [torch.randn(b, c, d, d, generator=gen).cuda() for c, d in zip(chans, dims)]
    ctot, n = sum(chans), len(chans)
    ld = headroom + ctot
    buf = torch.zeros(b, nv, ld, device="cuda")
    placed = [(torch.randn(b, nv, w, generator=gen).cuda(), c) for w, c in ((3, 0), (192, 3))] if fronts else []
    pooled(verts, cams, maps, buf[..., headroom:], ld if headroom else 0, placed, buf)
    save(name + "_features", buf if fronts else buf[..., headroom:])
    # backward, the gradient read out of a buffer as wide as the forward's
    gbuf = torch.zeros(b, nv, ld, device="cuda")
    gbuf[..., headroom:] = torch.randn(b, nv, ctot, generator=gen).cuda()
    gmaps = [torch.zeros_like(t) for t in maps] if maps_grad else []
    gverts = torch.zeros_like(verts)
    cdims = carray(ctypes.c_int, dims)
    ws_bytes = _lib.lib().geom_pool_features_bwd_workspace_bytes(b, nv, n, cdims)
    ws = torch.zeros((ws_bytes + 3) // 4, dtype=torch.int32, device="cuda")
    _lib.call("geom_pool_features_bwd_ld_f32", b, nv, verts.data_ptr(), cams[0].data_ptr(), cams[1].data_ptr(), n,
              carray(ctypes.c_void_p, [t.data_ptr() for t in maps]), carray(ctypes.c_int, chans), cdims, gbuf[..., headroom:].data_ptr(),
              ld if headroom else 0, carray(ctypes.c_void_p, [t.data_ptr() for t in gmaps]) if maps_grad else None, gverts.data_ptr(),
              ws.data_ptr(), ws_bytes)
    torch.cuda.synchronize()
    save(name + "_grad_verts", gverts)
    if not maps_grad:
        return
    offsets, ent_v, ent_w = sorted_lists(ws.cpu().numpy(), b, nv, dims)
    for tag, a in (("offsets", offsets), ("list_vertices", ent_v), ("list_weights", ent_w)):
        np.save(os.path.join(OUT, "%s_%s.npy" % (name, tag)), a)
    col = 0
    for l, (c, d) in enumerate(zip(chans, dims)):      # the float64 tests' bound: P = the identity maps of the size, pooled
        eye = torch.eye(d * d, device="cuda").view(1, d * d, d, d).expand(b, -1, -1, -1).contiguous()
        P = torch.zeros(b, nv, d * d, device="cuda")
        pooled(verts, cams, [eye], P, 0)
        g = gbuf[..., headroom + col:headroom + col + c].double()
        bound = 8 * EPS * torch.einsum("bvt,bvc->bct", P.double().abs(), g.abs()).view(b, c, d, d) + 1e-30
        np.save(os.path.join(GRADS, "%s_map%d.npy" % (name, l)), gmaps[l].cpu().numpy())
        np.save(os.path.join(GRADS, "%s_map%d_bound.npy" % (name, l)), bound.cpu().numpy())
        col += c


def main():
    global OUT, GRADS
    OUT = sys.argv[1]
    GRADS = sys.argv[2] if len(sys.argv) > 2 else OUT.rstrip("/") + "_mapgrads"
    os.makedirs(OUT, exist_ok=True)
    os.makedirs(GRADS, exist_ok=True)
    real = _lib.call

    def spy(name, *args):
        CALLS.append(name)
        return real(name, *args)
    _lib.call = spy
    ragged = {"four_maps": ((70, 130, 260, 5), (5, 9, 40, 1)), "two_maps": ((3, 64), (2, 13))}
    training = ((64, 128, 256, 512), (56, 28, 14, 7))
    for tag, (chans, dims) in sorted(ragged.items()):
        for headroom in (0, 7):
            case("ragged_%s_h%d" % (tag, headroom), ragged_inputs(), chans, dims, headroom)
    case("wide_2x1280", wide_inputs(), (1280, 1280), (14, 7))
    for headroom in (0, 195):
        case("training_h%d" % headroom, training_inputs(), *training, headroom)
    case("training_fronts", training_inputs(), *training, 195, fronts=True)
    case("training_verts_only", training_inputs(), *training, 195, maps_grad=False)
    torch.cuda.synchronize()
    CALLS.append("== batch_camera_info, 64 cameras")
    gen = torch.Generator(device="cpu").manual_seed(64)
    info = torch.rand(64, 3, generator=gen) * torch.tensor([720.0, 180.0, 1.0]) + torch.tensor([-360.0, -90.0, 0.7])
    cam_mat, cam_pos = utils.batch_camera_info(info.cuda())
    save("camera_mat", cam_mat)
    save("camera_pos", cam_pos)
    torch.cuda.synchronize()
    with open(os.path.join(OUT, "calls.txt"), "w") as fh:
        fh.write("\n".join(CALLS) + "\n")


if __name__ == "__main__":
    main()
