"""Every geom_dense_* entry of csrc/dense_gemm.hip, once, on seeded operands; each output as OUTDIR/<name>.npy.

    python tools/dump_dense_products.py OUTDIR

The sibling of tools/dump_tile_products.py (same `save` / `case`, same use): run from two checkouts on the same GPU, the two
directories must compare byte for byte (profiles/dense_gemm_refactor.txt).  The shapes walk the kernels' paths on 256 CUs:
fewer tiles than workgroups, the scalar loaders, leftover row-blocks, a second tile per workgroup, every tile height of the pair
launch and its fall-back to two launches.  OUTDIR/calls.txt lists the entry points of every case and the row geometry (tile
height rb, full tiles, leftover row-blocks) this machine's CU count gives it, so that a machine with another count shows."""
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dump_tile_products as tiles  # noqa: E402  (puts the repository on sys.path)
from dump_tile_products import case, save  # noqa: E402
from geometrics_amd import _lib, dense, layers, meshgen, optim, utils  # noqa: E402

SHAPES = [(83, 192, 192), (1000, 37, 48), (4000, 100, 96), (2562, 963, 192), (4100, 192, 192), (8200, 192, 192),
          (12300, 192, 192), (16400, 192, 192), (20496, 192, 192), (12369, 192, 192), (24592, 192, 192)]


def row_geometry(rows, ncw, cus):
    """dense_gemm.hip's row_geometry: (rb, full tiles, leftover row-blocks) of a rows-kernel launch."""
    n_rb, best, best_cost = (rows + 15) // 16, None, None
    for rb in (5, 6, 4, 3, 2, 1):
        n_tiles, left = divmod(n_rb, rb)
        if left * ncw > cus or (n_tiles == 0 and left == 0):
            continue
        grid = max(n_tiles, left * ncw) if n_tiles < cus else cus
        cost = max(-(-n_tiles // grid), 1) * rb * ncw + (1 if left else 0)
        if best_cost is None or cost < best_cost:
            best, best_cost = (rb, n_tiles, left), cost
    return best


def product_cases(rows, cin, c, cus):
    tag = "%d_%d_%d" % (rows, cin, c)
    gen = torch.Generator(device="cpu").manual_seed(rows + 7 * cin + 13 * c)
    x, w, g = tiles.rand(gen, rows, cin), 0.1 * tiles.rand(gen, cin, c), tiles.rand(gen, rows, c)
    want_bias = cin >= 48              # the column sums ride on the first full output tile
    case("%s: forward rb/tiles/left %s, dX (ncw %d) %s" % (tag, row_geometry(rows, 3, cus), 4 if cin > 192 else 3,
                                                           row_geometry(rows, 4 if cin > 192 else 3, cus)))
    save("fwd_" + tag, dense.forward(x, w))
    if c == 192:
        bias = 0.5 * tiles.rand(gen, c)
        out, sup = torch.zeros(rows, c, device="cuda"), torch.zeros(rows, 64, device="cuda")
        mask = torch.zeros(rows, c // 16, dtype=torch.int16, device="cuda")
        dense.forward_split(x, w, bias, 64, out, sup, mask)
        for name, t in (("out", out), ("sup", sup), ("mask", mask)):
            save("fwd_ksplit_%s_%s" % (name, tag), t)
    save("dx_" + tag, dense.backward_input(g, w))
    gw, gb = dense.backward_weight(x, g, want_bias)
    save("dw_" + tag, gw)
    if want_bias:
        save("db_" + tag, gb)
    ws = dense.weight_workspace(rows, cin, c, x.device).zero_()
    gx, gw, gb = torch.zeros(rows, cin, device="cuda"), torch.zeros(cin, c, device="cuda"), torch.zeros(c, device="cuda")
    dense.backward_pair(x, g, w, gx, ws, want_colsum=want_bias)
    dense.reduce([(rows, cin, c, ws, gw, gb if want_bias else None)])
    for name, t in (("dx", gx), ("dw", gw), ("db", gb)):
        save("pair_%s_%s" % (name, tag), t)


def joint_reduction_case():
    """geom_dense_reduce2_f32: two weight jobs and two column-sum jobs in one launch."""
    gen = torch.Generator(device="cpu").manual_seed(2)
    jobs = []
    for rows, cin, c in [(4000, 100, 96), (83, 192, 192)]:
        x, g = tiles.rand(gen, rows, cin), tiles.rand(gen, rows, c)
        ws = dense.weight_workspace(rows, cin, c, x.device).zero_()
        dense.backward_weight_partials(x, g, ws)
        jobs.append((rows, cin, c, ws, torch.zeros(cin, c, device="cuda")))
    sums = [(p, torch.zeros(p.shape[1], device="cuda")) for p in (tiles.rand(gen, 1288, 192), tiles.rand(gen, 7, 48))]
    ints = lambda seq: (ctypes.c_int * len(seq))(*seq)
    ptrs = lambda seq: (ctypes.c_void_p * len(seq))(*[t.data_ptr() for t in seq])
    case("joint reduction: 2 weight jobs, 2 column-sum jobs")
    _lib.check(_lib.status("geom_dense_reduce2_f32", 2, ints([j[0] for j in jobs]), ints([j[1] for j in jobs]),
                           ints([j[2] for j in jobs]), ptrs([j[3] for j in jobs]), ptrs([j[4] for j in jobs]), None, 2,
                           ptrs([p for p, _ in sums]), ints([p.shape[0] for p, _ in sums]), ints([p.shape[1] for p, _ in sums]),
                           ptrs([o for _, o in sums])), "geom_dense_reduce2_f32")
    for i, t in enumerate([j[4] for j in jobs] + [o for _, o in sums]):
        save("reduce2_%d" % i, t)


def adam_case():
    """Four iterations with the optimiser's step inside the end-of-pass reduction launch (geom_dense_reduce_adam_f32): the
    three-layer stack of tests/test_dense_gpu.py::test_adam_inside_the_backward_pass_equals_the_separate_launch."""
    V, Fc = meshgen.uv_sphere()
    adj = utils.adj_init(torch.from_numpy(Fc).cuda())["adj"]
    gen = torch.Generator(device="cpu").manual_seed(3)
    x, target = tiles.rand(gen, 4, V.shape[0], 40), tiles.rand(gen, 4, V.shape[0], 48)
    torch.manual_seed(3)
    stack = torch.nn.ModuleList([layers.Batch_Image_ZERON_GCNGCN(40, 48), layers.Batch_Image_ZERON_GCNGCN(48, 48),
                                 layers.Batch_Image_ZERON_GCNGCN(48, 48)]).cuda()
    opt = optim.FusedAdam(stack.parameters(), lr=1e-2)
    case("FusedAdam.in_backward, 4 iterations")
    for _ in range(4):
        opt.zero_grad()
        with layers.deferred_parameter_gradients(), opt.in_backward():
            h = x
            for layer in stack:
                h = layer(h, adj, F.relu)
            ((h - target) ** 2).mean().backward()
        assert getattr(opt, "_stepped_in_backward", False), "the reduction launch must have taken the step"
        opt.step()
    tiles.CALLS.append("step_count %d" % opt.step_count)
    for i, t in enumerate(list(stack.parameters()) + [p.grad for p in stack.parameters()] + opt.exp_avg + opt.exp_avg_sq):
        save("adam_%02d" % i, t)


def main():
    tiles.OUT = sys.argv[1]
    os.makedirs(tiles.OUT, exist_ok=True)
    real = _lib.status

    def spy(name, *args, **kw):                    # _lib.call goes through _lib.status too
        tiles.CALLS.append(name)
        return real(name, *args, **kw)
    _lib.status = spy
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles.CALLS.append("compute units: %d" % cus)
    for rows, cin, c in SHAPES:
        product_cases(rows, cin, c, cus)
    joint_reduction_case()
    adam_case()
    torch.cuda.synchronize()
    with open(os.path.join(tiles.OUT, "calls.txt"), "a") as fh:
        fh.write("\n".join(tiles.CALLS) + "\n")


if __name__ == "__main__":
    main()
