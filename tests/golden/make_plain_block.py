"""Generate tests/golden/plain_block.npz: the reference's BatchNorm-free MeshDeformationBlock (models.py:138-201) on its
Image_ZERON_GCNGCN layers (old_GEOMetrics/layers.py:106-149) in FLOAT64 on the CPU, one forward + backward per case.

    python tests/golden/make_plain_block.py

`import make_golden` provides the stubs, the reference's path and save().  The two classes are compiled from the reference
files where they lie, by line range (the recipe of make_face_split.legacy_functions, line numbers asserted); nothing of the
files is written to the repository.  Parameters and inputs are regenerated from seeds (tests/deform_plain_helpers.py).

Cases (inputs features [V,3], pooled [V,192]; cotangents g_features [V,192], g_coords [V,3]):

    sphere482        MeshDeformationBlock(195) on the 482-vertex UV sphere, ReLU
    split181         the same block on the adjacency split_ico1_two_rounds.npz stores after round 2 (V = 181), ReLU
    split181_smooth  ... with F.relu patched to the identity
    layer40          ONE Image_ZERON_GCNGCN(40, 48) layer with ReLU on the 181-vertex adjacency (input [V,40], cotangent [V,48])

Stored per case: seed, input checksums, float64 weighted checksums of every full output and gradient, ROWS sampled rows of the
192-wide tensors, the [V,3] tensors whole, WROWS sampled rows of the weight gradients of gc1, gc2, gc7, gc13; the layer case
whole.  Asserted on the reference alone: an fp32 CPU evaluation of the same reference block lies within a QUARTER of each bar
the fp32 routes are held to (forward 2e-5, gradients 5e-5 of the tensor's scale).  Should a stored quantity miss that, its bar
becomes four times the fp32 reference's error rounded up to one digit, stored as `bar.<name>` and read by the tests -- never
anything derived from the kernels."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stubs, reference path, save())
from make_golden import meshgen, ref_utils, t  # noqa: E402

sys.path.insert(0, os.path.join(make_golden.ROOT, "tests"))
import deform_plain_helpers as dph  # noqa: E402

LINES = {"Image_ZERON_GCNGCN": ("old_GEOMetrics/layers.py", (106, 149)), "MeshDeformationBlock": ("models.py", (138, 203))}


def reference_classes():
    scope = {"torch": torch, "nn": torch.nn, "F": torch.nn.functional, "math": math, "Module": torch.nn.Module,
             "Parameter": torch.nn.Parameter}
    for name, (rel, expected) in LINES.items():
        path = os.path.join(make_golden.REF, rel)
        with open(path) as f:
            lines = f.readlines()
        start = next(i for i, l in enumerate(lines) if l.startswith("class %s(" % name))
        end = next((i for i in range(start + 1, len(lines)) if lines[i].startswith(("def ", "class "))), len(lines))
        assert (start + 1, end + 1) == expected, (name, start + 1, end + 1)
        exec(compile("\n" * start + "".join(lines[start:end]), path, "exec"), scope)
    return scope


def one_digit_up(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e) * 10 ** e


def make_plain_block():
    ref = reference_classes()
    arrays = {}
    V, Fc = meshgen.uv_sphere()
    adj = ref_utils.adj_init(t(Fc))["adj"].numpy()
    r, c = np.nonzero(adj)
    arrays.update({"uv_sphere_482.adj_rows": r.astype(np.int16), "uv_sphere_482.adj_cols": c.astype(np.int16),
                   "uv_sphere_482.adj_vals": adj[r, c].astype(np.float32), "uv_sphere_482.nv": np.int64(adj.shape[0])})
    for case, (mesh, relu, seed) in dph.BLOCK_CASES.items():
        A32 = dph.case_adjacency(mesh, arrays)
        nv = A32.shape[0]
        inputs = dph.case_inputs(seed, nv)
        out = dict(mesh=np.array(mesh), nv=np.int64(nv), seed=np.int64(seed), relu=np.bool_(relu))
        for name, a in inputs.items():
            out["in_ck." + name] = np.float64(a.astype(np.float64).sum())
        block = dph.fill_plain_parameters(ref["MeshDeformationBlock"](195), seed)
        names = sorted(n for n, _ in block.named_parameters())
        out["param_names"] = np.array(names)
        out["in_ck.params"] = np.array([float(dict(block.named_parameters())[n].detach().double().sum()) for n in names])
        full = dph.run_block(block.double(), inputs, {"adj": torch.from_numpy(A32).double()}, relu, torch.float64)
        rows_v = dph.sampled_rows(seed, nv, A32)
        wrows = {i: dph.weight_rows(seed, i, 195 if i == 1 else 192) for i in dph.WLAYERS}
        out["rows_v"] = rows_v
        for i in dph.WLAYERS:
            out["wrows.gc%d" % i] = wrows[i]
        out.update({k: v.astype(np.float32) for k, v in dph.block_stored(full, rows_v, wrows).items()})
        out["ck_names"], out["ck"] = dph.checksums(full)
        out["ck_names"] = np.array(out["ck_names"])
        arrays.update({"%s.%s" % (case, k): v for k, v in out.items()})
        # the fp32 CPU evaluation of the SAME reference block against what was just stored
        block32 = dph.fill_plain_parameters(ref["MeshDeformationBlock"](195), seed)
        full32 = dph.run_block(block32, inputs, {"adj": torch.from_numpy(A32)}, relu, torch.float32)
        for name, err in sorted(dph.errors_against(arrays, case, full32).items()):
            bar = dph.bar_of(None, case, name)
            print("%-16s %-28s fp32 reference %.2e (quarter bar %.2e)" % (case, name, err, bar / 4))
            if err > bar / 4:
                arrays["%s.bar.%s" % (case, name)] = np.float64(one_digit_up(4 * err))
                print("    -> bar.%s = %g" % (name, one_digit_up(4 * err)))
    # the single layer
    case, mesh, seed, n_in, n_out = dph.LAYER_CASE
    A32 = dph.case_adjacency(mesh)
    nv = A32.shape[0]
    layer = dph.fill_plain_parameters(ref["Image_ZERON_GCNGCN"](n_in, n_out), seed).double()
    inputs = dph.case_inputs(seed, nv, n_in, 1, n_out)
    x = torch.from_numpy(inputs["features"]).double().requires_grad_(True)
    y = layer(x, {"adj": torch.from_numpy(A32).double()}, torch.nn.functional.relu)
    (y * torch.from_numpy(inputs["g_features"]).double()).sum().backward()
    arrays.update({case + ".seed": np.int64(seed), case + ".in_ck.features": np.float64(inputs["features"].astype(np.float64).sum()),
                   case + ".out": y.detach().numpy().astype(np.float32), case + ".grad.input": x.grad.numpy().astype(np.float32),
                   case + ".grad.weight1": layer.weight1.grad.numpy().astype(np.float32),
                   case + ".grad.bias": layer.bias.grad.numpy().astype(np.float32)})
    make_golden.save("plain_block", **arrays)


if __name__ == "__main__":
    make_plain_block()
