"""Every launch that runs a tile product of csrc/mfma_tiles.h, once, on seeded inputs; each output as OUTDIR/<name>.npy.

    python tools/dump_tile_products.py OUTDIR

Run from two checkouts on the same GPU, the two directories must compare byte for byte (cmp, or `diff -r`): the check behind a
change that may move no result bit (profiles/mfma_tiles_refactor.txt).  The shapes are the smallest the tests use; OUTDIR/calls.txt
lists the library entry points every case went through, so that a case that silently took another route shows.
geom_gemm_f32's 16-deep instantiation is chosen by GEOM_GEMM_TILE, which the library reads once per process: that case runs in
a child process."""
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))      # (the plain block's cases)
from geometrics_amd import _lib, aggregation, deform, dense, encoder, fused, layers, meshgen, models, utils  # noqa: E402
import deform_plain_helpers as dph  # noqa: E402

OUT = None
CALLS = []


def save(name, t):
    t = t.detach().contiguous().cpu()
    np.save(os.path.join(OUT, name + ".npy"), t.view(torch.int32).numpy() if t.dtype == torch.float32 else t.numpy())


def case(name):
    torch.cuda.synchronize()
    CALLS.append("== " + name)


def rand(gen, *shape):
    return torch.randn(*shape, generator=gen).cuda()


def mesh(kind):
    V, Fc = meshgen.uv_sphere() if kind == "uv482" else meshgen.icosphere(2)
    adj = utils.adj_init(torch.from_numpy(np.ascontiguousarray(Fc)).cuda())["adj"]
    return V.shape[0], adj, layers.adjacency_csr(adj)


def gemm_forms(tag, shapes):
    for m, n, k in shapes:
        gen = torch.Generator(device="cpu").manual_seed(m + 7 * n + 13 * k)
        x, w, wt, xt = rand(gen, m, k), rand(gen, k, n), rand(gen, n, k), rand(gen, k, m)
        case("%s %dx%dx%d" % (tag, m, n, k))
        save("%s_xw_%d_%d_%d" % (tag, m, n, k), dense.gemm(x, w))
        save("%s_gwt_%d_%d_%d" % (tag, m, n, k), dense.gemm(x, wt, trans_b=True))
        save("%s_xtg_%d_%d_%d" % (tag, m, n, k), dense.gemm(xt, w, trans_a=True))


def gemm_cases():
    gemm_forms("gemm", [(70, 60, 3), (324, 150, 120), (130, 300, 250)])
    gen = torch.Generator(device="cpu").manual_seed(1446)
    x, g = rand(gen, 1446, 60), rand(gen, 1446, 60)
    need = int(_lib.lib().geom_gemm_workspace_floats(60, 60, 1446))
    assert need > 0, "the weight-gradient case must take the split over the summed index"
    case("gemm dw 60x60 over 1446 rows, %d workspace floats" % need)
    save("gemm_dw_60_60_1446", dense.gemm(x, g, trans_a=True, workspace=torch.empty(need, device="cuda")))


def encoder_cases():
    nv, _, csr = mesh("ico162")
    b, rows = 2, 2 * nv
    for cin, cout in [(3, 60), (120, 150), (300, 50)]:
        gen = torch.Generator(device="cpu").manual_seed(100 * cin + cout)
        s, w = rand(gen, rows, cin), rand(gen, cin, cout) / cin ** 0.5
        identity = cin == 3
        bias = None if identity else 0.3 * rand(gen, cin)
        k, act = (0, aggregation.ACT_NONE) if identity else (cin // 10, aggregation.ACT_ELU)
        x = torch.zeros(rows, cin, device="cuda")
        case("encoder fwd %d->%d" % (cin, cout))
        save("enc_fwd_%d_%d" % (cin, cout), encoder.layer_forward(s, csr, k, bias, act, w, b, nv, x_out=x))
        save("enc_fwd_x_%d_%d" % (cin, cout), x)
        g = rand(gen, rows, cout)
        head = cout == 50                 # the head's adjoint tail: no activation in front of its max
        saved = None if head else torch.nn.functional.elu(rand(gen, rows, cout))
        t = torch.zeros(rows, cout, device="cuda")
        case("encoder bwd %d->%d" % (cout, cin))
        save("enc_bwd_%d_%d" % (cin, cout), encoder.layer_backward(g, saved, csr, cout // 10, aggregation.ACT_NONE if head else aggregation.ACT_ELU,
                                                                   w, b, nv, t_out=t))
        save("enc_bwd_t_%d_%d" % (cin, cout), t)


def zn_layer_cases():
    nv, _, csr = mesh("ico162")
    C, K = 192, 64
    for b, act, n_out in [(5, 1, 192), (2, 2, 96)]:       # 810 rows: a ragged last row-block and leftover row-blocks
        gen = torch.Generator(device="cpu").manual_seed(200 + b)
        s_prev, bias, w = rand(gen, b, nv, C), 0.3 * rand(gen, C), 0.1 * rand(gen, C, n_out)
        mask = torch.zeros(b * nv * 16, dtype=torch.int16, device="cuda") if act == 1 else None
        wt = torch.zeros(n_out, C, device="cuda")
        case("zn layer fwd b=%d act=%d n_out=%d" % (b, act, n_out))
        x, s = fused.layer_forward(s_prev, bias, csr, K, act, w, mask=mask, wt_out=wt)
        for name, t in (("x", x), ("s", s), ("wt", wt), ("mask", mask)):
            if t is not None:
                save("zn_fwd_%s_b%d_a%d" % (name, b, act), t)
    for b, act, head in [(5, 1, True), (5, 1, False), (2, 2, False)]:
        gen = torch.Generator(device="cpu").manual_seed(300 + b + (7 if head else 0))
        out = rand(gen, b, nv, C)
        wt = (0.1 * rand(gen, C, C)).t().contiguous()
        mask = None
        if act == 1:                   # sign words in the aggregation kernel's layout, from the forward kernel itself
            out = torch.empty(b, nv, C, device="cuda")
            mask = layers.aggregate_forward(rand(gen, b, nv, C), None, csr, K, 1, out, want_mask=True)
        gp = rand(gen, b, nv, 3) if head else None
        grad_out = None if head else rand(gen, b, nv, C)
        partial = torch.zeros(fused.partial_rows(b, nv), C, device="cuda")
        case("zn layer bwd b=%d act=%d head=%d" % (b, act, head))
        g_out, grad_in = fused.layer_backward(grad_out, out if act == 2 else None, mask, csr, K, act, wt, colsum_partial=partial,
                                              grad_pos=gp, head_scale=0.01, shape=(b, nv, C))
        for name, t in (("g", g_out), ("gin", grad_in), ("colsum", partial)):
            save("zn_bwd_%s_b%d_a%d_h%d" % (name, b, act, head), t)


def deform_cases():
    nv, adj, _ = mesh("uv482")
    for tag, b, chain, wide in [("layers", 3, False, False), ("chain", 3, True, False), ("wide", 17, True, True)]:
        torch.manual_seed(16)
        block = models.BatchMeshDeformationBlock(3 + 197, nv).cuda().train()
        gen = torch.Generator(device="cpu").manual_seed(b)
        feats, pooled = rand(gen, b, nv, 3).requires_grad_(True), rand(gen, b, nv, 197).requires_grad_(True)
        deform.chain, deform.wide = chain, wide
        case("deform block %s b=%d" % (tag, b))
        f, c = block(feats, pooled, adj)
        (f * torch.linspace(-1, 1, f.shape[-1], device=f.device)).sum().add((c * c).sum()).backward()
        outs = [f, c, feats.grad, pooled.grad] + [p.grad for p in block.parameters() if p.grad is not None]
        outs += [getattr(block, "bn%d" % i).running_var for i in range(1, 14)]
        for i, t in enumerate(outs):
            save("deform_%s_%02d" % (tag, i), t)
    block.eval()
    gen = torch.Generator(device="cpu").manual_seed(1)
    feats, pooled = rand(gen, 1, nv, 3), rand(gen, 1, nv, 197)
    case("deform block eval b=1")
    with torch.no_grad():
        f, c = block(feats, pooled, adj)
    save("deform_eval_00", f)
    save("deform_eval_01", c)
    for b in (18, 40):                 # 543 and 1205 row-blocks on 512 workgroups: later row-blocks behind the slice a workgroup holds
        gen = torch.Generator(device="cpu").manual_seed(b)
        feats, pooled = rand(gen, b, nv, 3), rand(gen, b, nv, 197)
        case("deform block eval b=%d" % b)
        with torch.no_grad():
            f, c = block(feats, pooled, adj)
        save("deform_eval_b%d_00" % b, f)
        save("deform_eval_b%d_01" % b, c)
    plain_block_cases()
    plain_launch_cases()


def plain_block_cases():
    """models.MeshDeformationBlock forward + backward on the 482-vertex sphere and the 519-vertex split mesh with its 65-entry
    row: every output, input gradient and parameter gradient."""
    for which in ("b", "d"):
        adj = torch.from_numpy(dph.launch_adjacency(which)).cuda()
        nv = adj.shape[0]
        block = dph.fill_plain_parameters(models.MeshDeformationBlock(195), 50 + ord(which)).cuda()
        gen = torch.Generator(device="cpu").manual_seed(ord(which))
        feats, pooled = rand(gen, nv, 3).requires_grad_(True), rand(gen, nv, 192).requires_grad_(True)
        case("plain block %s nv=%d" % (which, nv))
        f, c = block(feats, pooled, adj)
        (f * torch.linspace(-1, 1, f.shape[-1], device=f.device)).sum().add((c * c).sum()).backward()
        outs = [f, c, feats.grad, pooled.grad] + [p.grad for _, p in sorted(block.named_parameters()) if p.grad is not None]
        for i, t in enumerate(outs):
            save("plain_block_%s_%02d" % (which, i), t)


def plain_launch_cases():
    """Single plain launches at 18 x 482 rows (543 row-blocks on 512 workgroups: some workgroups take a second row-block), a
    residual at a pitch wider than 192, with a product and with the head, forward and backward."""
    adj = torch.from_numpy(dph.launch_adjacency("b")).cuda()
    csr = layers.adjacency_csr(adj)
    b, nv = 18, csr.nv
    gen = torch.Generator(device="cpu").manual_seed(1800)
    s, bias, w, w_head = rand(gen, b, nv, 192), 0.1 * rand(gen, 192), 0.1 * rand(gen, 192, 192), 0.1 * rand(gen, 192, 3)
    res = rand(gen, b, nv, 259)[:, :, :192]
    w2, wts = deform.pack_weights([w])
    z, x, s_out = (torch.zeros(b, nv, 192, device="cuda") for _ in range(3))
    case("plain fwd b=18 product")
    deform.plain_layer_forward(s, bias, csr, True, res, 0.5, z_out=z, x_out=x, w_next=w2[0], s_out=s_out)
    x_last, s_head = torch.zeros(b, nv, 192, device="cuda"), torch.zeros(b, nv, 3, device="cuda")
    case("plain fwd b=18 head")
    deform.plain_layer_forward(s, bias, csr, True, res, 0.5, x_out=x_last, w_head=w_head, s_head=s_head)
    for name, t in (("z", z), ("x", x), ("s", s_out), ("x_last", x_last), ("s_head", s_head)):
        save("plain_fwd_%s" % name, t)
    nrb = (b * nv + 15) // 16
    dz_up, g2, g, ds_head = rand(gen, b, nv, 192), rand(gen, b, nv, 259)[:, :, 67:], rand(gen, b, nv, 259)[:, :, :192], rand(gen, b, nv, 3)
    dz, ds_up, grad_res, colsum = (torch.zeros(*shape, device="cuda") for shape in [(b, nv, 192)] * 3 + [(nrb, 192)])
    case("plain bwd b=18 product")
    deform.plain_layer_backward((b, nv, 192), csr, z, True, True, 0.5, dz, dz_up=dz_up, ds_up=ds_up, wt_up=wts[0], g2=g2,
                                grad_res=grad_res, colsum=colsum)
    for name, t in (("dz", dz), ("ds_up", ds_up), ("grad_res", grad_res), ("colsum", colsum)):
        save("plain_bwd_%s" % name, t)
    dw_head = torch.zeros(nrb, 576, device="cuda")
    case("plain bwd b=18 head")
    deform.plain_layer_backward((b, nv, 192), csr, z, True, True, 0.5, dz, g=g, g2=g2, grad_res=grad_res, colsum=colsum,
                                ds_head=ds_head, w_head=w_head, x_top=x, dw_head=dw_head)
    for name, t in (("dz", dz), ("grad_res", grad_res), ("colsum", colsum), ("dw_head", dw_head)):
        save("plain_bwd_top_%s" % name, t)


def main():
    global OUT
    OUT = sys.argv[1]
    os.makedirs(OUT, exist_ok=True)
    real = _lib.call

    def spy(name, *args):
        CALLS.append(name)
        return real(name, *args)
    _lib.call = spy
    if os.environ.get("GEOM_GEMM_TILE") == "16":          # the child: the 16-deep instantiation only
        gemm_forms("gemm16", [(324, 150, 120)])
    else:
        gemm_cases()
        encoder_cases()
        zn_layer_cases()
        deform_cases()
        torch.cuda.synchronize()
        subprocess.run([sys.executable, os.path.abspath(__file__), OUT], env=dict(os.environ, GEOM_GEMM_TILE="16"), check=True)
    torch.cuda.synchronize()
    with open(os.path.join(OUT, "calls.txt"), "a") as fh:
        fh.write("\n".join(CALLS) + "\n")


if __name__ == "__main__":
    main()
