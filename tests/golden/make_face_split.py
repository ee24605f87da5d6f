"""Generate tests/golden/split_*.npz: the reference's adaptive face splitting (old_GEOMetrics/utils.py: adj_init l.112,
normalize_adj l.140, calc_face_list l.158, calc_curve l.431, split_info l.481) run on the CPU, inputs and results only.

    python tests/golden/make_face_split.py

`import make_golden` provides the stubs (torch.Tensor.cuda is the identity), the reference's path and save().  The legacy module
does not import under python 3, so the five functions are compiled from the reference file where they lie, by line range (the
recipe of make_golden.legacy_point_to_line, line numbers asserted); nothing of the file is written to the repository.

Cases (meshgen.jittered_batch(V, 1, sigma)[0] of an icosphere; two chained rounds of calc_curve + split_info each, so that in
round 2 the active list is no longer the identity and `faces` holds dead rows):

    split_ico1_threshold    icosphere(1), sigma .15, angle 70      split_ico1_two_rounds   icosphere(1), sigma .15, angle 40
    split_ico1_fallback     icosphere(1), sigma .02, angle 70      split_ico2_two_rounds   icosphere(2), sigma .1,  angle 40
    split_482_pole          the reference's 482.obj, three hand-made lists: all 32 faces of one pole's fan and 5 scattered
                            faces (shuffled), two faces (the reference cannot split ONE: its numpy indexing with a
                            one-element tensor drops a dimension, utils.py:580-587), and every face (a permutation)

Conditions asserted on the reference alone, so that no test passes or fails by round-off:
  * a threshold round returns the SAME selection at angle - 0.05, angle and angle + 0.05, and selects between 3 faces and all;
    where the nominal angle of a round does not, the round's angle moves in steps of 0.2 degrees until it does (stored: rN.angle);
  * a fallback round (fewer than 3 faces above the angle) has a gap of more than 1e-4 rad between the third and the fourth
    largest curvature of a float64 restatement, and the reference's three are the restatement's three.

Stored per round r (keys r1.*, r2.*; the pole case: pole.*, two.*, all.*): the inputs verts [V,3] / features [V,5] fp32, faces,
face_list, `splitting` (the reference's order), `selected` (sorted) and `fallback`; the outputs faces, face_list (the reference's
is float64; stored int64), the non-zeros of adj (rows, cols, fp32 values; adj_orig is 1 at exactly these places, asserted), verts, features;
grad_seed -- the cotangent of (verts, features) is helpers.seeded_input([grad_seed, 2 / 3], shape) -- and the reference's
input gradients; curvature64, the float64 restatement."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stubs, reference path, save())

sys.path.insert(0, os.path.join(make_golden.ROOT, "tests"))
import helpers  # noqa: E402

C = 5
LINES = {"adj_init": (112, 140), "normalize_adj": (140, 158), "calc_face_list": (158, 182), "calc_curve": (431, 481),
         "split_info": (481, 642)}
# case -> (icosphere level, sigma, angle, seed, expected selections per round: a count, or "fallback")
CASES = {"split_ico1_threshold": (1, .15, 70, 3101, (57, "fallback")),
         "split_ico1_fallback": (1, .02, 70, 3102, ("fallback",)),
         "split_ico1_two_rounds": (1, .15, 40, 3103, (71, 68)),
         "split_ico2_two_rounds": (2, .1, 40, 3104, (303, 278))}


def legacy_functions():
    import scipy.sparse as sp
    path = os.path.join(make_golden.REF, "old_GEOMetrics", "utils.py")
    with open(path) as f:
        lines = f.readlines()
    scope = {"torch": torch, "np": np, "sp": sp}
    for name, expected in LINES.items():
        start = next(i for i, l in enumerate(lines) if l.startswith("def %s(" % name))
        end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(("def ", "class ")))
        assert (start + 1, end + 1) == expected, (name, start + 1, end + 1)
        exec(compile("\n" * start + "".join(lines[start:end]), path, "exec"), scope)
    return scope


def curvature64(verts, faces, face_list):
    """calc_curve's curvature (radians) restated in float64."""
    v, f, fl = np.asarray(verts, np.float64), np.asarray(faces, np.int64), np.asarray(face_list, np.int64)
    p1, p2, p3 = v[f[:, 1]], v[f[:, 0]], v[f[:, 2]]
    n = np.cross(p2 - p1, p3 - p1)
    with np.errstate(all="ignore"):
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        own = n[fl[:, 0, 2]]
        eps = np.float64(np.float32(.00001))
        terms = [np.arccos(np.clip((own * n[fl[:, j, 0]]).sum(1), -1.0 + eps, 1.0 - eps)) for j in range(3)]
    return (terms[0] + terms[1] + terms[2]) / 3.0


def sparse(prefix, dense):
    dense = np.asarray(dense)
    r, c = np.nonzero(dense)
    return {prefix + ".rows": r.astype(np.int32), prefix + ".cols": c.astype(np.int32), prefix + ".vals": dense[r, c].astype(np.float32)}


def one_split(ref, info, verts, feats, splitting, seed):
    """The reference's split_info on fp32 leaves, with a seeded cotangent: (arrays to store, next info, next verts, next feats)."""
    v, f = make_golden.t(verts, grad=True), make_golden.t(feats, grad=True)
    sel = torch.from_numpy(np.asarray(splitting, np.int64))
    new_info, v2, f2 = ref["split_info"](info, v, f, sel, len(splitting))
    gv, gf = helpers.seeded_input([seed, 2], tuple(v2.shape)), helpers.seeded_input([seed, 3], tuple(f2.shape))
    ((v2 * torch.from_numpy(gv)).sum() + (f2 * torch.from_numpy(gf)).sum()).backward()
    fl = np.asarray(new_info["face_list"])
    assert (fl == np.round(fl)).all()
    out = {"in.verts": verts, "in.features": feats, "in.faces": np.asarray(info["faces"], np.int64),
           "in.face_list": np.asarray(info["face_list"], np.int64), "splitting": np.asarray(splitting, np.int64),
           "faces": np.asarray(new_info["faces"], np.int64), "face_list": fl.astype(np.int64), "nv": np.int64(v2.shape[0]),
           "verts": v2.detach().numpy(), "features": f2.detach().numpy(), "grad_seed": np.int64(seed),
           "grad.verts": v.grad.numpy(), "grad.features": f.grad.numpy()}
    pattern, values = sparse("adj_orig", new_info["adj_orig"]), sparse("adj", new_info["adj"].numpy())
    assert (pattern["adj_orig.vals"] == 1).all() and all((pattern["adj_orig." + k] == values["adj." + k]).all() for k in ("rows", "cols"))
    out.update({"adj.rows": values["adj.rows"], "adj.cols": values["adj.cols"], "adj.vals": values["adj.vals"]})
    return out, new_info, out["verts"], out["features"]


def select(ref, case, verts, info, angle, expected):
    """The reference's calc_curve with the generator's conditions; (splitting as the reference returns it, arrays to store)."""
    tv = make_golden.t(verts)
    sel = ref["calc_curve"](tv, info, angle).numpy().astype(np.int64)
    c64 = curvature64(verts, info["faces"], info["face_list"])
    nfa = len(info["face_list"])
    above = int((c64 * 180.0 / np.pi > angle).sum())
    if expected == "fallback":
        assert above < 3 and sel.shape == (3,), (case, above, sel)
        order = np.argsort(-c64, kind="stable")
        gap = float(c64[order[2]] - c64[order[3]])
        assert gap > 1e-4, (case, gap)
        assert sorted(sel.tolist()) == sorted(order[:3].tolist()), (case, sel, order[:3])
        print("%-24s fallback %s, gap third/fourth %.2e rad" % (case, sel.tolist(), gap))
    else:
        # the selection has to be the same 0.05 degrees either side; where it is not at the nominal angle, the round's angle moves
        # in steps of 0.2 degrees until it is, and the fixture records the angle used
        nominal = angle
        for step in (0, 1, -1, 2, -2, 3, -3, 4, -4):
            angle = nominal + 0.2 * step
            sel, lo, hi = (ref["calc_curve"](tv, info, a).numpy().astype(np.int64) for a in (angle, angle - 0.05, angle + 0.05))
            if sel.shape == lo.shape == hi.shape and (sel == lo).all() and (sel == hi).all():
                break
        else:
            raise AssertionError("%s: no angle near %g with a selection stable to +-0.05 degrees" % (case, nominal))
        above = int((c64 * 180.0 / np.pi > angle).sum())
        assert 3 <= sel.size < nfa and sel.size == above, (case, sel.size, above, nfa)
        assert angle != nominal or sel.size == expected, (case, sel.size, expected)
        assert (np.diff(sel) > 0).all()
        print("%-24s %d of %d faces above %g degrees" % (case, sel.size, nfa, angle))
    return sel, {"selected": np.sort(sel), "fallback": np.int64(expected == "fallback"), "angle": np.float64(angle),
                 "curvature64": c64}


def start_info(ref, faces, nv):
    info = ref["adj_init"](np.asarray(faces), nv)
    info["face_list"] = ref["calc_face_list"](np.asarray(faces))
    assert info["face_list"].shape == (len(faces), 3, 3)
    return info


def make_ico_case(ref, case, level, sigma, angle, seed, expected):
    V, F = make_golden.meshgen.icosphere(level)
    verts = make_golden.meshgen.jittered_batch(V, 1, sigma=sigma)[0]
    feats = helpers.seeded_input([seed, 1], (verts.shape[0], C))
    info = start_info(ref, F, verts.shape[0])
    arrays = {"level": np.int64(level), "sigma": np.float64(sigma), "seed": np.int64(seed), "rounds": np.int64(len(expected))}
    for r, want in enumerate(expected, 1):
        sel, picked = select(ref, case, verts, info, angle, want)
        out, info, verts, feats = one_split(ref, info, verts, feats, sel, seed + 10 * r)
        out.update(picked)
        arrays.update({"r%d.%s" % (r, k): v for k, v in out.items()})
    make_golden.save(case, **arrays)


def make_pole_case(ref):
    ref_info, verts = make_golden.ref_utils.load_initial(os.path.join(make_golden.REF, "482.obj"))
    faces, verts = ref_info["faces"].numpy().astype(np.int64), verts.numpy().astype(np.float32)
    assert (faces == helpers.golden("adj_482")["faces"]).all()      # the committed fixture's faces
    nv, seed = verts.shape[0], 3105
    feats = helpers.seeded_input([seed, 1], (nv, C))
    degree = np.bincount(faces.reshape(-1), minlength=nv)
    pole = int(np.argmax(degree))
    fan = np.nonzero((faces == pole).any(1))[0]
    assert degree[pole] == 32 and fan.size == 32
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(len(faces)), fan)
    lists = {"pole": rng.permutation(np.concatenate([fan, rng.choice(rest, 5, replace=False)])),
             "two": np.array([417, 3]), "all": rng.permutation(len(faces))}
    arrays = {"pole_vertex": np.int64(pole), "seed": np.int64(seed)}
    for k, (name, splitting) in enumerate(lists.items()):
        assert np.unique(splitting).size == splitting.size
        out, _, _, _ = one_split(ref, start_info(ref, faces, nv), verts, feats, splitting.astype(np.int64), seed + 10 * (k + 1))
        if name != "pole":             # the inputs are the pole list's
            out = {key: v for key, v in out.items() if not key.startswith("in.")}
        arrays.update({"%s.%s" % (name, key): v for key, v in out.items()})
        print("split_482_pole %-5s S = %d" % (name, splitting.size))
    make_golden.save("split_482_pole", **arrays)


def make_face_split():
    ref = legacy_functions()
    for case, (level, sigma, angle, seed, expected) in CASES.items():
        make_ico_case(ref, case, level, sigma, angle, seed, expected)
    make_pole_case(ref)
    for name in list(CASES) + ["split_482_pole"]:
        size = os.path.getsize(os.path.join(HERE, name + ".npz"))
        assert size < 300 * 1024, (name, size)


if __name__ == "__main__":
    make_face_split()
