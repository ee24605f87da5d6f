"""Time one calc_curve + split_info at the 482-vertex template (960 faces, C = 192 features) -- a report, not a gate:

  project     utils.calc_curve + utils.split_info (csrc/face_split.hip; one host read: the number of selected faces)
  reference   the reference's formulation (old_GEOMetrics/utils.py:431-634) RESTATED here in torch on the same GPU, its numpy
              parts on the host as the reference runs them: eager curvature ops and a host np.where; index tables, a dense
              float64 (V+S)^2 adjacency and its normalisation in numpy; the results copied back to the device

for two selections: the fixture's hand-made pole list (37 faces: the whole fan of a pole + 5) and a threshold selection
(calc_curve at the median curvature of the jittered template: about half of the faces).  HIP events around each call after
warm-up; median and (min .. max) over --iters calls.  The two sides' tables are compared before anything is timed.

    python tools/time_face_split.py [--iters 50] [--out profiles/face_split.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geometrics_amd import utils  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
C = 192


def restated_calc_curve(verts, info, angle):
    """Eager torch ops on the device, the selection on the host (np.where), the indices copied back."""
    faces = torch.LongTensor(info["faces"]).cuda()
    fl = torch.LongTensor(info["face_list"]).cuda()
    p1, p2, p3 = (torch.index_select(verts, 0, faces[:, k]) for k in (1, 0, 2))
    normals = torch.cross(p2 - p1, p3 - p1, dim=1)
    normals = normals / torch.norm(normals, p=2, dim=1).view(-1, 1)
    own = torch.index_select(normals, 0, fl[:, 0, 2])
    terms = [torch.sum(own * torch.index_select(normals, 0, fl[:, j, 0]), dim=1).clamp(-1.0 + 1e-5, 1.0 - 1e-5).acos().view(-1, 1)
             for j in range(3)]
    curvature = torch.mean(torch.cat(terms, dim=1), dim=1)
    picked = np.where((curvature * 180 / np.pi > angle).cpu().numpy())[0]
    if picked.shape[0] < 3:
        return curvature.topk(3, sorted=False)[1]
    return torch.LongTensor(picked).cuda()


def restated_split_info(info, verts, features, splitting, number):
    """The tables in numpy on the host (a dense float64 adjacency among them), the new rows with torch ops on the device."""
    adj, faces, fl = info["adj_orig"], np.asarray(info["faces"]), np.asarray(info["face_list"])
    sp = splitting.cpu().numpy()
    nv, nft, nfa, s = adj.shape[0], faces.shape[0], fl.shape[0], sp.shape[0]
    counter = np.zeros(nfa)
    counter[sp] = 1
    keep = np.where(counter == 0)[0]
    own_split, own_keep = fl[sp, 0, 2], fl[keep, 0, 2]
    children = nft + np.arange(s).reshape(-1, 1) + s * np.arange(3).reshape(1, -1)
    position = np.zeros((nft, 3), np.int64)
    position[own_split] = children
    position[own_keep] = own_keep.reshape(-1, 1)
    across = lambda rows, j: position[rows[:, j, 0], rows[:, j, 1]]
    kept = np.stack([np.stack((across(fl[keep], j), fl[keep][:, j, 1], own_keep), axis=1) for j in range(3)], axis=1)
    rows = fl[sp]
    blocks = []
    for k in range(3):
        slots = []
        for j in range(3):
            if j == k:
                slots.append(np.stack((across(rows, j), rows[:, j, 1], children[:, k]), axis=1))
            else:
                slots.append(np.stack((children[:, j], np.full(s, k), children[:, k]), axis=1))
        blocks.append(np.stack(slots, axis=1))
    new_fl = np.concatenate([kept] + blocks)
    x, y, z = (faces[own_split][:, k] for k in range(3))
    n = nv + np.arange(number)
    new_faces = np.concatenate((faces, np.stack((x, y, n), 1), np.stack((n, y, z), 1), np.stack((x, n, z), 1)))
    both = torch.cat((verts, features), dim=1)
    both = torch.cat((both, both[x] / 3 + both[y] / 3 + both[z] / 3))
    new_adj = np.zeros((nv + number, nv + number))
    new_adj[np.tile(n, 4), np.concatenate((n, x, y, z))] = 1
    new_adj[:nv, :nv] = adj
    new_adj = np.maximum(new_adj, new_adj.T)
    normalised = torch.FloatTensor(new_adj * np.power(new_adj.sum(1), -1).reshape(-1, 1)).cuda()
    return {"adj": normalised, "adj_orig": new_adj, "faces": new_faces, "face_list": new_fl}, both[:, :3], both[:, 3:]


def timed(fn, iters):
    times = []
    for _ in range(iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) * 1e3)
    return "%9.1f (%.1f .. %.1f)" % (statistics.median(times), min(times), max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_split.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(GOLDEN, "split_482_pole.npz"))
    faces, face_list, pole = g["pole.in.faces"], g["pole.in.face_list"], g["pole.splitting"]
    rng = np.random.default_rng(482)
    verts = torch.from_numpy((g["pole.in.verts"] + 0.01 * rng.standard_normal(g["pole.in.verts"].shape)).astype(np.float32)).to(dev)
    feats = torch.from_numpy(rng.standard_normal((verts.shape[0], C)).astype(np.float32)).to(dev)
    info = utils.adj_init(torch.from_numpy(faces).to(dev))
    info["face_list"] = utils.calc_face_list(info["faces"])
    assert np.array_equal(info["face_list"].cpu().numpy(), face_list)
    host = {"adj_orig": info["adj_orig"].cpu().numpy().astype(np.float64), "faces": faces, "face_list": face_list}
    from geometrics_amd import ops
    angle = float(np.median(ops.face_curvature(verts, info["faces"], info["face_list"]).cpu().numpy()) * 180 / np.pi)
    pole_dev = torch.from_numpy(pole).to(dev)

    def project(selection):
        sel = utils.calc_curve(verts, info, angle)
        sel = pole_dev if selection == "pole" else sel
        return utils.split_info(info, verts, feats, sel, sel.numel())

    def reference(selection):
        sel = restated_calc_curve(verts, host, angle)
        sel = pole_dev if selection == "pole" else sel
        return restated_split_info(host, verts, feats, sel, sel.numel())

    lines = ["# tools/time_face_split.py --iters %d on %s" % (args.iters, torch.cuda.get_device_name(0)),
             "# one calc_curve + split_info at V = %d, F = %d, C = %d; us per call between HIP events: median (min .. max) of %d "
             "calls after warm-up" % (verts.shape[0], faces.shape[0], C, args.iters),
             "%-10s %6s %32s %32s" % ("selection", "S", "project", "reference's formulation")]
    for selection in ("pole", "threshold"):
        (ia, va, fa), (ib, vb, fb) = project(selection), reference(selection)
        # (the new rows to round-off only: on the GPU torch divides by a scalar by multiplying with its reciprocal, so the eager
        # x/3 + y/3 + z/3 there is not the bits of the same expression on the CPU, which the project's kernel reproduces)
        same = (np.array_equal(ia["faces"].cpu().numpy(), ib["faces"]) and np.array_equal(ia["face_list"].cpu().numpy(), ib["face_list"])
                and torch.equal(ia["adj"], ib["adj"]) and torch.allclose(va, vb, rtol=1e-6, atol=1e-7)
                and torch.allclose(fa, fb, rtol=1e-6, atol=1e-6))
        if not same:
            raise SystemExit("time_face_split.py: the two sides disagree at the %s selection" % selection)
        for _ in range(5):
            project(selection), reference(selection)
        lines.append("%-10s %6d %32s %32s" % (selection, va.shape[0] - verts.shape[0], timed(lambda: project(selection), args.iters),
                                              timed(lambda: reference(selection), args.iters)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
