"""Generate tests/golden/pooling_matrix.npz: the reference's projection-matrix pooling (old_GEOMetrics/utils.py: pooling l.379)
run on the CPU in fp32 and in float64, inputs and results only.

    python tests/golden/make_matrix_pooling.py

`import make_golden` provides the stubs (torch.Tensor.cuda is the identity), the reference's path and save().  The legacy module
does not import under python 3, so the function is compiled from the reference file where it lies, by line range (the recipe of
make_face_split.py, line numbers asserted); nothing of the file is written to the repository.

Inputs (tests/pool_matrix_ref.py builds them; the GPU tests build the same): the three vertex sets of the ragged pooling tests
(meshes 0 and 1: 101 vertices at three radii, the outer one partly off the image; mesh 2: 70 vertices), one image each; matrices
of family E (equivalent to the cameras (35, 20, 1.2), (250, -30, 0.8), (60, 30, 1.0)) and G (E with every entry perturbed by up to
3 %, seeded, row 2 = 1e30: the reference computes q2 and drops it); maps "two_maps" ((3, 64) channels at 2 x 2 and 13 x 13) and
"thin" ((6, 3, 5, 2) channels at 5, 9, 40, 1), seeded N(0, 1), as is the cotangent.

Cases.  A case's map gradients are as large as its maps -- 10 828 values for two_maps, dense -- in fp32 AND float64, so the full
cross (3 meshes x 2 families x 2 shapes) would be 1.4 MB; stored (396 KB) is the set below, chosen so that every mesh meets every family
on the thin shape (its 1 x 1 map, its 40 x 40 map, its 3 / 5 / 6 / 2 channels: 35 KB a case) and two_maps (190 KB a case) is run
once, on the general family and on mesh 1 -- the mesh whose outer shell is clamped on both axes:
    thin: E and G on meshes 0, 1, 2;    two_maps: G on mesh 1.
The GPU tests run the full cross against the float64 restatement, which test_matrix_pooling_host.py pins to these cases (and,
for family E on every shape, to oracle.ref_ops.pool_features with the cameras).

Conditions asserted here, on the reference's float64 run and the restatement pinned to it alone:
  * at most 2 % of a mesh's vertices lie within 1e-3 texels of a texel line or clamp edge of any map of the case (helpers.POOL_NEAR
    / POOL_MAX_LEFT_OUT); if a case exceeds the cap, change G's seed (pool_matrix_ref.G_SEED), not the cap;
  * mesh 1 has vertices clamped on both axes of every map (exactly zero gradient rows) under both families.

Stored per case `<family>.m<mesh>.<shape>`: .verts [V,3] and .proj [4,4] fp32 (the maps and the cotangent are
pool_matrix_ref.maps_and_gradient(shape, V): host generator), then the reference's .feats32 [V, sum C], .gv32 [V,3], .gm32.<l>
[C_l,d,d] and the float64 run's .feats64, .gv64, .gm64.<l>; .left_out, .zero_rows: the counts of the two conditions."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stubs, reference path, save())

sys.path.insert(0, os.path.join(make_golden.ROOT, "tests"))
import helpers  # noqa: E402
import pool_matrix_ref as pm  # noqa: E402

LINES = {"pooling": (379, 431)}
CASES = [(f, m, "thin") for f in "EG" for m in range(3)] + [("G", 1, "two_maps")]


def legacy_pooling():
    path = os.path.join(make_golden.REF, "old_GEOMetrics", "utils.py")
    with open(path) as f:
        lines = f.readlines()
    torch.cuda.LongTensor = torch.LongTensor          # the reference casts indices with .type(torch.cuda.LongTensor)
    scope = {"torch": torch, "np": np}
    for name, expected in LINES.items():
        start = next(i for i, l in enumerate(lines) if l.startswith("def %s(" % name))
        end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(("def ", "class ")))
        assert (start + 1, end + 1) == expected, (name, start + 1, end + 1)
        exec(compile("\n" * start + "".join(lines[start:end]), path, "exec"), scope)
    return scope["pooling"]


def reference_run(pooling, maps, verts, matrix, cot, dtype):
    v = verts.detach().clone().to(dtype).requires_grad_(True)
    mm = [t[0].detach().clone().to(dtype).requires_grad_(True) for t in maps]
    feats = pooling(mm, v, matrix.to(dtype))
    got = torch.autograd.grad(feats, [v] + mm, cot[0].to(dtype))
    return feats.detach().numpy(), got[0].numpy(), [g.numpy() for g in got[1:]]


def main():
    pooling = legacy_pooling()
    meshes = pm.meshes()
    out, both_axes = {}, {}
    for fam, m, shape in CASES:
        key = "%s.m%d.%s" % (fam, m, shape)
        verts, proj = meshes[m], pm.family(fam)[0][m]
        maps, cot = pm.maps_and_gradient(shape, verts.shape[0])
        out[key + ".verts"], out[key + ".proj"] = verts.numpy(), proj.numpy()
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            feats, gv, gm = reference_run(pooling, maps, verts, proj, cot, dtype)
            assert feats.dtype == gv.dtype == (np.float32 if tag == "32" else np.float64)
            out[key + ".feats" + tag], out[key + ".gv" + tag] = feats, gv
            for l, g in enumerate(gm):
                out["%s.gm%s.%d" % (key, tag, l)] = g
        grad, _, _, near = pm.pool_vertex_gradient(maps, verts[None], proj[None], cot)
        scale = np.abs(out[key + ".gv64"]).max()
        assert np.abs(grad[0] - out[key + ".gv64"]).max() <= 1e-12 * scale, key       # (the conditions are the reference's)
        left_out = int((near[0] < helpers.POOL_NEAR).sum())
        assert left_out <= helpers.POOL_MAX_LEFT_OUT * verts.shape[0], "%s: %d of %d vertices near a texel line" % (key, left_out, verts.shape[0])
        zero_rows = int((out[key + ".gv64"] == 0).all(-1).sum())
        both_axes[(fam, m, shape)] = zero_rows
        out[key + ".left_out"], out[key + ".zero_rows"] = np.int64(left_out), np.int64(zero_rows)
        print("%-18s left out %d of %d, zero rows %d" % (key, left_out, verts.shape[0], zero_rows))
    assert all(n >= 1 for (f, m, s), n in both_axes.items() if m == 1), both_axes
    make_golden.save("pooling_matrix", **out)


if __name__ == "__main__":
    main()
