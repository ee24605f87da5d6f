"""Dev helper: the surface loss of a training batch of B = 16 meshes that each own their faces -- ONE call of
utils.ragged_point_to_surface on the union mesh (draw, Chamfer scan, ragged point-to-triangle scan, closest point, three sums;
scatter backward) against the loop of B per-mesh utils.batch_point_to_surface calls at b = 1 (existing code: the baseline; each
its own draw / scan / finalize / gather chain) -- forward + backward, eager, between HIP events.

Shapes: the reference's 482-vertex template (tests/golden/adj_482.npz, 960 faces) and the mesh it becomes when every face is
split (tests/golden/split_482_pole.npz `all`: 1442 vertices, 2880 active faces), 16 jittered copies each, 3000 sampled + 3000
ground-truth points per mesh.  The loop is given its best case: the 16 meshes share one face tensor, so its per-face-list tables
(face order, vertex-face lists) are built once, which a batch of 16 different topologies would not allow.  The two arms alternate
inside every round of one process (same box, same clocks); per shape the table gives the median of the rounds, each arm's own
range over the rounds and whether the ragged call wins by more than that spread: median(loop) - median(ragged) >
max(range of ragged, range of loop).  profiles/ragged_loss.txt is this tool's output.

    python tools/time_ragged_loss.py [--rounds 7] [--seconds 0.6] [--out FILE]

--backward: the ragged call's two backward routes instead -- ordered (finalize + one gather launch, the default) against scatter
(GEOM_RAGGED_BACKWARD=scatter: zero-fill + fp32 atomics), forward + backward, eager and as one captured graph each; and the three
stages of the cascade stacked into ONE weighted call on a union of 3 B meshes against three calls with float weights, eager and
captured.  All arms of a shape alternate inside every round; median and range over the rounds.  The output is appended to
profiles/ragged_loss_backward.txt behind the resource tables.

    python tools/time_ragged_loss.py --backward [--rounds 7] [--seconds 0.6] [--out FILE]
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
from geometrics_amd import meshgen, ops, utils

GOLDEN = os.path.join(ROOT, "tests", "golden")
B, NUM, N_GT = 16, 3000, 3000


def shapes():
    g = np.load(os.path.join(GOLDEN, "adj_482.npz"))
    yield "482 unsplit", g["verts"], g["faces"]
    g = np.load(os.path.join(GOLDEN, "split_482_pole.npz"))
    yield "1442 split", g["all.verts"], g["all.faces"][g["all.face_list"][:, 0, 2]]       # the active faces


def events_us(work, count):
    work()                                                    # (warm: the arm's first call after the other's)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(count):
        work()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / count


def captured(step):
    """`step` (a forward + backward that keeps nothing of its autograd graph) as one captured graph's replay."""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph.replay


def backward_routes(args, gpu):
    stage_weights = (0.2, 0.2, 2.0)
    lines = ["# ragged surface loss (point to surface), %d meshes with their own faces, %d sampled + %d gt points per mesh, forward + backward,"
             % (B, NUM, N_GT),
             "# microseconds per call; %s; rounds = %d, all arms of a shape alternating in every round, >= %.1f s of timed work per arm"
             % (torch.cuda.get_device_name(gpu), args.rounds, args.seconds),
             "# ordered = finalize + ONE gather launch (no float atomics, the default); scatter = GEOM_RAGGED_BACKWARD=scatter (zero-fill +",
             "# fp32 atomics); stacked = the three stages (weights .2 / .2 / 2) as ONE weighted call on a union of %d meshes; 3 calls = one" % (3 * B),
             "# call per stage with a float weight; graph = the same step replayed from one captured graph",
             "# median over the rounds (range = max - min of the arm's rounds)"]
    bench.settle_clocks(gpu, 200)
    ops.manual_seed(41, gpu)
    for name, verts, faces in shapes():
        nv, nf = verts.shape[0], faces.shape[0]
        gt = torch.from_numpy(meshgen.gt_cloud(B, N_GT)).to(gpu)
        faces_one = torch.from_numpy(faces.astype(np.int64)).to(gpu)
        faces_union = torch.cat([faces_one + m * nv for m in range(B)])
        face_mesh = torch.arange(B, device=gpu).repeat_interleave(nf)
        stages = [torch.from_numpy(meshgen.jittered_batch(verts.astype(np.float32), B, first=s * B)).to(gpu).reshape(-1, 3).clone()
                  .requires_grad_(True) for s in range(3)]
        union = stages[0]
        stacked = torch.cat([s.detach() for s in stages]).requires_grad_(True)
        faces_stacked = torch.cat([faces_union + s * B * nv for s in range(3)])
        mesh_stacked = torch.cat([face_mesh + s * B for s in range(3)])
        gt_stacked = torch.cat((gt, gt, gt))
        w_stacked = torch.tensor(stage_weights, device=gpu).repeat_interleave(B)

        def one_call(route):
            def step():
                ops.ragged_backward = route
                union.grad = None
                utils.ragged_point_to_surface(union, faces_union, face_mesh, gt, num=NUM).backward()
            return step

        def three_calls():
            ops.ragged_backward = "ordered"
            for s, w in zip(stages, stage_weights):
                s.grad = None
                utils.ragged_point_to_surface(s, faces_union, face_mesh, gt, num=NUM, weight=w).backward()

        def stacked_call():
            ops.ragged_backward = "ordered"
            stacked.grad = None
            utils.ragged_point_to_surface(stacked, faces_stacked, mesh_stacked, gt_stacked, num=NUM, weight=w_stacked).backward()

        arms = [("ordered", one_call("ordered")), ("scatter", one_call("scatter")), ("3 calls", three_calls), ("stacked", stacked_call)]
        arms += [("ordered graph", captured(one_call("ordered"))), ("scatter graph", captured(one_call("scatter")))]
        ops.ragged_backward = "ordered"
        arms += [("3 calls graph", captured(three_calls)), ("stacked graph", captured(stacked_call))]
        for _, work in arms:
            for _ in range(3):
                work()
        torch.cuda.synchronize()
        probe = max(events_us(work, 3) for _, work in arms)
        count = max(5, int(args.seconds * 1e6 / (probe * args.rounds)) + 1)
        rounds = [[events_us(work, count) for _, work in arms] for _ in range(args.rounds)]
        ops.ragged_backward = "ordered"
        lines.append("%s: %d verts, %d faces per mesh" % (name, nv, nf))
        for i, (arm, _) in enumerate(arms):
            times = [r[i] for r in rounds]
            lines.append("    %-14s %9.1f us  (range %6.1f)" % (arm, statistics.median(times), max(times) - min(times)))
        print("\n".join(lines[-len(arms) - 1:]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.6, help="timed work per arm and shape, over all rounds")
    ap.add_argument("--out", default=None)
    ap.add_argument("--backward", action="store_true", help="time the ragged call's backward routes and the stacked stages instead")
    args = ap.parse_args()
    gpu = torch.device("cuda:0")
    if args.backward:
        text = "\n".join(backward_routes(args, gpu)) + "\n"
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text)
        return
    lines = ["# surface loss (point to surface) of %d meshes with their own faces, forward + backward, eager, microseconds per batch; %s;"
             % (B, torch.cuda.get_device_name(gpu)),
             "# %d sampled + %d gt points per mesh; rounds = %d, arms alternating, >= %.1f s of timed work per arm" % (NUM, N_GT, args.rounds,
                                                                                                                   args.seconds),
             "# ragged = ONE utils.ragged_point_to_surface call on the union mesh; loop = %d utils.batch_point_to_surface calls at b = 1" % B,
             "# medians over the rounds; range = max - min of an arm's rounds; ratio = median loop / median ragged;",
             "# 'wins' = median loop - median ragged > max(range ragged, range loop)",
             "%-12s %7s %7s %10s %10s %10s %10s %7s %5s" % ("shape", "verts", "faces", "ragged us", "range", "loop us", "range", "ratio", "wins")]
    bench.settle_clocks(gpu, 200)
    ops.manual_seed(41, gpu)
    for name, verts, faces in shapes():
        nv, nf = verts.shape[0], faces.shape[0]
        copies = torch.from_numpy(meshgen.jittered_batch(verts.astype(np.float32), B)).to(gpu)
        gt = torch.from_numpy(meshgen.gt_cloud(B, N_GT)).to(gpu)
        faces_one = torch.from_numpy(faces.astype(np.int64)).to(gpu)
        info = {"faces": faces_one}
        singles = [copies[m:m + 1].clone().requires_grad_(True) for m in range(B)]
        union = copies.reshape(-1, 3).clone().requires_grad_(True)
        faces_union = torch.cat([faces_one + m * nv for m in range(B)])
        face_mesh = torch.arange(B, device=gpu).repeat_interleave(nf)

        def ragged_step():
            union.grad = None
            utils.ragged_point_to_surface(union, faces_union, face_mesh, gt, num=NUM).backward()

        def loop_step():
            for m, v in enumerate(singles):
                v.grad = None
                utils.batch_point_to_surface(v, info, gt[m:m + 1], num=NUM).backward()

        for work in (ragged_step, loop_step):
            for _ in range(3):
                work()
        torch.cuda.synchronize()
        probe = max(events_us(ragged_step, 3), events_us(loop_step, 3))      # steps per round: --seconds of work per arm in all
        count = max(5, int(args.seconds * 1e6 / (probe * args.rounds)) + 1)
        rounds = [(events_us(ragged_step, count), events_us(loop_step, count)) for _ in range(args.rounds)]
        rs, ls = [r for r, _ in rounds], [l for _, l in rounds]
        mr, ml = statistics.median(rs), statistics.median(ls)
        rr, rl = max(rs) - min(rs), max(ls) - min(ls)
        lines.append("%-12s %7d %7d %10.1f %10.1f %10.1f %10.1f %7.3f %5s" % (name, nv, nf, mr, rr, ml, rl, ml / mr,
                                                                            "yes" if ml - mr > max(rr, rl) else "no"))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
