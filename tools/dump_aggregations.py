"""Every aggregation kernel of csrc/zn_gcn.hip, once, on seeded inputs through the C ABI; each output as OUTDIR/<name>.npy.

    python tools/dump_aggregations.py OUTDIR

Run with two builds of the library on the same GPU, the two directories must compare byte for byte (cmp, or `diff -r`): the
check behind a change to that file that may move no result bit (profiles/zn_gcn_refactor.txt).  Per case: output, input
gradient, sign mask, positions, the raw rows of bias-gradient partials and the reduced bias gradient -- of the CSR kernel and
of the table kernel the shape is routed to.  Cases: the grid of tests/test_aggregate_kernels_gpu.py on its two graphs (table
widths 16 and 8, both with CSR tails), the headline shapes 8 x 2562 x 192 and 16 x 482 x 192 at k = 64, and the encoder's
widths on the ragged batch of tests/test_aggregate_any_gpu.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from geometrics_amd import _lib as L, layers, meshgen, ragged, utils  # noqa: E402

OUT = None
SCALE = 0.01


def save(name, t):
    t = t.detach().contiguous().cpu()
    np.save(os.path.join(OUT, name + ".npy"), t.view(torch.int32).numpy() if t.dtype == torch.float32 else t.numpy())


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def from_faces(faces):
    return layers.adjacency_csr(utils.adj_init(gpu(faces))["adj"])


def ragged_batch():
    verts, faces = [], []
    for i, level in enumerate([2, 3, 2, 4, 3]):
        V, Fc = meshgen.icosphere(level)
        verts.append(gpu(meshgen.jittered_batch(V, 1, first=i)[0]))
        faces.append(gpu(Fc))
    return ragged.RaggedMeshBatch.from_faces(verts, faces).csr


def backward(tag, entry, b, nv, c, rows, *args):
    """One backward entry point on NaN-prefilled buffers: gradient, reduced bias gradient, the partial rows it wrote."""
    grad, gb = torch.full((b, nv, c), float("nan"), device="cuda"), torch.full((c,), float("nan"), device="cuda")
    scr = torch.full((L.lib().geom_zn_gcn_bwd_scratch_floats(b, nv, c),), float("nan"), device="cuda")
    L.call(entry, *args, grad.data_ptr(), gb.data_ptr(), scr.data_ptr())
    assert 0 < rows * c <= scr.numel()
    for name, t in (("grad", grad), ("gb", gb), ("partial", scr[:rows * c])):
        save("%s_%s" % (tag, name), t)


def case(graph, csr, b, c, k, act, mode="saved"):
    """mode: where the table kernel's backward takes act' from -- the saved output, the sign mask, or head mode."""
    nv, w = csr.nv, csr.ell_w
    tag = "%s_b%d_c%d_k%d_a%d_%s" % (graph, b, c, k, act, mode)
    gen = torch.Generator(device="cpu").manual_seed(1000 * c + 10 * k + act)
    sup, bias, gout = (torch.randn(*s, generator=gen).cuda() for s in ((b, nv, c), (c,), (b, nv, c)))
    base, grad_pos = (torch.randn(b, nv, 3, generator=gen).cuda() for _ in range(2))
    out = torch.full_like(sup, float("nan"))
    rows = lambda ell_w: int(L.lib().geom_zn_gcn_bwd_partial_rows(b, nv, c, k, ell_w))
    if mode == "saved":
        L.call("geom_zn_gcn_aggregate_fwd_f32", b, nv, c, k, csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(),
               sup.data_ptr(), bias.data_ptr(), act, out.data_ptr())
        save(tag + "_csr_out", out)
        backward(tag + "_csr", "geom_zn_gcn_aggregate_bwd_f32", b, nv, c, rows(0), b, nv, c, k, csr.rowptr_t.data_ptr(),
                 csr.col_t.data_ptr(), csr.val_t.data_ptr(), gout.data_ptr(), out.data_ptr() if act else None, act)
    if not w:
        return
    over, over_t = csr.over or (None, None, None), csr.over_t or (None, None, None)
    table = (csr.ell_col.data_ptr(), csr.ell_val.data_ptr()) + tuple(L.ptr(t) for t in over)
    table_t = (csr.ell_col_t.data_ptr(), csr.ell_val_t.data_ptr()) + tuple(L.ptr(t) for t in over_t)
    masked = mode == "mask" or (mode == "head" and act == 1)
    mask = torch.zeros(L.lib().geom_zn_gcn_relu_mask_words(b, nv, c, k), dtype=torch.int16, device="cuda") if masked else None
    out.fill_(float("nan"))
    if mode == "head":
        pos = torch.full_like(base, float("nan"))
        L.call("geom_zn_gcn_aggregate_ell_head_fwd_f32", b, nv, c, k, w, *table, sup.data_ptr(), bias.data_ptr(), act,
               out.data_ptr(), L.ptr(mask), base.data_ptr(), SCALE, pos.data_ptr())
        save(tag + "_pos", pos)
    else:
        L.call("geom_zn_gcn_aggregate_ell_fwd_f32", b, nv, c, k, w, *table, sup.data_ptr(), bias.data_ptr(), act,
               out.data_ptr(), L.ptr(mask))
    save(tag + "_out", out)
    if masked:
        save(tag + "_mask", mask)
    if mode == "head":
        backward(tag, "geom_zn_gcn_aggregate_ell_head_bwd_f32", b, nv, c, rows(w), b, nv, c, k, w, *table_t, grad_pos.data_ptr(),
                 SCALE, L.ptr(mask), act)
    else:
        backward(tag, "geom_zn_gcn_aggregate_ell_bwd_f32", b, nv, c, rows(w), b, nv, c, k, w, *table_t, gout.data_ptr(),
                 out.data_ptr() if (act and not masked) else None, L.ptr(mask), act)


def main():
    global OUT
    OUT = sys.argv[1]
    os.makedirs(OUT, exist_ok=True)
    wide = layers.adjacency_csr(gpu(meshgen.hub_ring_adjacency()))
    template = from_faces(np.load(os.path.join(ROOT, "tests", "golden", "adj_482.npz"))["faces"])
    assert wide.ell_w == 16 and template.ell_w == 8 and wide.over and template.over
    for graph, csr in (("wide16", wide), ("template", template)):
        for act in (0, 1, 2):
            for c, k in ((72, 24), (120, 12), (52, 6), (50, 5), (7, 3)):
                case(graph, csr, 2, c, k, act)
        for act, mode in ((1, "mask"), (1, "head"), (0, "head")):
            case(graph, csr, 2, 72, 24, act, mode)
    sphere = from_faces(meshgen.icosphere(4)[1])
    for graph, csr, b in (("ico2562", sphere, 8), ("template", template, 16)):      # the headline shapes
        for act, mode in ((0, "saved"), (1, "saved"), (2, "saved"), (1, "mask"), (1, "head"), (0, "head")):
            case(graph, csr, b, 192, 64, act, mode)
    batch = ragged_batch()
    for c in (60, 120, 150, 200, 210, 250, 300, 50):                                # the encoder's layers, k = c // 10
        for act in (2, 0):
            case("ragged", batch, 1, c, c // 10, act)
    torch.cuda.synchronize()
    print("%d files in %s" % (len(os.listdir(OUT)), OUT))


if __name__ == "__main__":
    main()
