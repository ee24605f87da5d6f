"""Dev helper: the adaptive split of a training batch of B = 16 meshes that each own their topology -- ONE eager
utils.ragged_calc_curve + utils.ragged_split_info on the union mesh (C = 192 features) against the two ways the per-mesh code can
do the same work:

  loop    16 x (utils.calc_curve + utils.split_info), one mesh at a time (16 host reads, 16 x 2 dense [V+S,V+S] matrices);
  one     utils.calc_curve + utils.split_info on the union as ONE mesh: the one-workgroup launches over the whole union, two dense
          [n,n] matrices and ONE batch-wide fallback -- not the same selection where a mesh has fewer than 3 hits, so it is timed
          for its kernels only, and only where its matrices are affordable (the first shape: [7712+S]^2).

Shapes: the reference's 482-vertex template (tests/golden/adj_482.npz, 960 faces) and the mesh it becomes when every face is
split (tests/golden/split_482_pole.npz `all`: 1442 vertices, 2880 active faces of 3840), 16 jittered copies each; the threshold
is the median curvature of the union, so about half of the faces split.  The loop is given its best case: the 16 meshes share
one info dict, so the CSR of its adjacency is read once.  The arms alternate inside every round of one process; per shape the
table gives the median of the rounds, each arm's own range over the rounds and whether the ragged call wins by more than that
spread: median(loop) - median(ragged) > max(range of ragged, range of loop).  Below it: the new launches' own times between HIP
events.  profiles/ragged_split.txt is this tool's output.

    python tools/time_ragged_split.py [--rounds 7] [--seconds 0.6] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from geometrics_amd import meshgen, ops, ragged, utils

GOLDEN = os.path.join(ROOT, "tests", "golden")
B, C = 16, 192


def shapes():
    """(name, verts, every face ever made, face_list, whether the union's dense matrices are affordable)."""
    g = np.load(os.path.join(GOLDEN, "adj_482.npz"))
    faces = g["faces"].astype(np.int64)
    yield "482 unsplit", g["verts"], faces, utils.calc_face_list(torch.from_numpy(faces)).numpy(), True
    g = np.load(os.path.join(GOLDEN, "split_482_pole.npz"))
    yield "1442 split", g["all.verts"], g["all.faces"].astype(np.int64), g["all.face_list"].astype(np.int64), False


def events_us(work, count):
    work()                                                    # (warm: the arm's first call after the other's)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(count):
        work()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.6, help="timed work per arm and shape, over all rounds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gpu = torch.device("cuda:0")
    lines = ["# one adaptive split (curvature, selection, split; C = %d features) of %d meshes with their own topology, forward, eager, "
             "microseconds per batch; %s;" % (C, B, torch.cuda.get_device_name(gpu)),
             "# rounds = %d, arms alternating, >= %.1f s of timed work per arm" % (args.rounds, args.seconds),
             "# ragged = ONE utils.ragged_calc_curve + utils.ragged_split_info on the union; loop = %d x (utils.calc_curve + utils.split_info);" % B,
             "# one = utils.calc_curve + utils.split_info on the union as one mesh (dense [n,n] matrices, one batch-wide fallback: its kernels only)",
             "# medians over the rounds; range = max - min of an arm's rounds; ratio = median loop / median ragged;",
             "# 'wins' = median loop - median ragged > max(range ragged, range loop)",
             "%-12s %6s %6s %6s %10s %9s %10s %9s %10s %9s %7s %5s" % ("shape", "verts", "rows", "S", "ragged us", "range", "loop us", "range",
                                                                    "one us", "range", "ratio", "wins")]
    kernels = []
    bench.settle_clocks(gpu, 200)
    for name, verts, faces, face_list, dense_fits in shapes():
        nv, nft, nfa = verts.shape[0], faces.shape[0], face_list.shape[0]
        verts_all = torch.from_numpy(meshgen.jittered_batch(verts.astype(np.float32), B, sigma=0.01)).to(gpu)
        feats_all = torch.from_numpy(np.random.default_rng(482).standard_normal((B, nv, C)).astype(np.float32)).to(gpu)
        faces_one, list_one = torch.from_numpy(faces).to(gpu), torch.from_numpy(face_list).to(gpu)
        active = faces_one[list_one[:, 0, 2]]
        info_one = {"faces": faces_one, "face_list": list_one, "adj_orig": utils.calc_adj(active)}
        # the union: vertices, faces and rows of mesh m shifted by m times the mesh's counts
        faces_union = torch.cat([faces_one + m * nv for m in range(B)])
        shift = torch.tensor([1, 0, 1], device=gpu).view(1, 1, 3)
        list_union = torch.cat([list_one + m * nft * shift for m in range(B)]).contiguous()
        vert_mesh = torch.arange(B, device=gpu).repeat_interleave(nv)
        active_union = faces_union[list_union[:, 0, 2]]
        info = {"faces": faces_union, "face_list": list_union, "face_mesh": ragged.face_mesh(faces_union, vert_mesh).contiguous(),
                "vert_mesh": vert_mesh, "csr": ragged.csr_from_faces(active_union, B * nv), "b": B}
        verts_union, feats_union = verts_all.reshape(-1, 3).contiguous(), feats_all.reshape(-1, C).contiguous()
        curvature = ops.face_curvature(verts_union, faces_union, list_union)
        angle = float(np.median(curvature.cpu().numpy()) * 180 / np.pi)
        info_dense = dict(info_one, faces=faces_union, face_list=list_union, adj_orig=utils.calc_adj(active_union)) if dense_fits else None

        def ragged_step():
            splitting, _ = utils.ragged_calc_curve(verts_union, info, angle)
            return utils.ragged_split_info(info, verts_union, feats_union, splitting)

        def loop_step():
            out = []
            for m in range(B):
                selected = utils.calc_curve(verts_all[m], info_one, angle)
                out.append(utils.split_info(info_one, verts_all[m], feats_all[m], selected, selected.numel()))
            return out

        def one_step():
            selected = utils.calc_curve(verts_union, info_dense, angle)
            return utils.split_info(info_dense, verts_union, feats_union, selected, selected.numel())

        # the two routes split the same faces: mesh m's rows of the union's new vertices are the loop's
        _, v_union, _ = ragged_step()
        split_counts = utils.ragged_calc_curve(verts_union, info, angle)[1].tolist()
        looped = loop_step()
        if split_counts != [v.shape[0] - nv for _, v, _ in looped]:
            raise SystemExit("time_ragged_split.py: the union and the loop split different numbers of faces on %s" % name)
        start = B * nv
        for m, (_, v, _) in enumerate(looped):
            if not torch.equal(v_union[start:start + split_counts[m]], v[nv:]):
                raise SystemExit("time_ragged_split.py: the union's new vertices of mesh %d are not the loop's on %s" % (m, name))
            start += split_counts[m]
        arms = [ragged_step, loop_step] + ([one_step] if dense_fits else [])
        for work in arms:
            for _ in range(3):
                work()
        torch.cuda.synchronize()
        probe = max(events_us(work, 3) for work in arms)      # steps per round: --seconds of work per arm in all
        count = max(5, int(args.seconds * 1e6 / (probe * args.rounds)) + 1)
        rounds = [[events_us(work, count) for work in arms] for _ in range(args.rounds)]
        cols = list(zip(*rounds))
        med, rng = [statistics.median(c) for c in cols], [max(c) - min(c) for c in cols]
        one = "%10.1f %9.1f" % (med[2], rng[2]) if dense_fits else "%10s %9s" % ("-", "-")
        lines.append("%-12s %6d %6d %6d %10.1f %9.1f %10.1f %9.1f %s %7.3f %5s" % (
            name, B * nv, B * nfa, sum(split_counts), med[0], rng[0], med[1], rng[1], one, med[1] / med[0],
            "yes" if med[1] - med[0] > max(rng[0], rng[1]) else "no"))
        print(lines[-1], flush=True)
        # the new launches alone
        row_list, row_off = ragged.group_rows(list_union, info["face_mesh"], B)
        splitting = utils.ragged_calc_curve(verts_union, info, angle)[0].contiguous()
        select = lambda: ops.select_faces_ragged(curvature, angle, row_list, row_off)
        index = lambda: ops.split_index_ragged(faces_union, list_union, splitting, B * nv, vert_mesh, info["face_mesh"])
        old_select = lambda: ops.select_faces(curvature, angle)
        old_index = lambda: ops.split_index(faces_union, list_union, splitting, B * nv)
        times = []
        for work in (select, old_select, index, old_index):
            runs = [events_us(work, 50) for _ in range(args.rounds)]
            times.append("%8.1f (%.1f .. %.1f)" % (statistics.median(runs), min(runs), max(runs)))
        kernels.append("%-12s %28s %28s %28s %28s" % ((name,) + tuple(times)))
    lines += ["#", "# the launches alone on the same unions, us per call between HIP events (allocations included), median (min .. max) of %d x 50 calls:"
              % args.rounds,
              "# select: geom_face_select_ragged_f32 (2 launches, a workgroup per mesh) / geom_face_select_f32 (1 workgroup over the union);",
              "# index: geom_face_split_index_ragged (zero-fill + 4 launches over chunks) / geom_face_split_index (1 workgroup over the union)",
              "%-12s %28s %28s %28s %28s" % ("shape", "select ragged", "select one workgroup", "index ragged", "index one workgroup")] + kernels
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
