"""Dev helper: the image-feature pooling of a training batch of B = 16 meshes that each own their vertex count -- ONE call of
utils.ragged_pooling on the union mesh (one launch forward, two backward) against the loop of B per-mesh utils.batched_pooling
calls at b = 1 (existing code: the baseline; B launches forward, 2 B backward) -- forward + backward with the maps and the
positions wanting a gradient, eager, between HIP events.

Shapes: the four VGG maps (64, 128, 256, 512) x (56, 28, 14, 7) of 16 images; the union of 16 x 482 vertices (the reference's
template, tests/golden/adj_482.npz) and of 16 x 1442 (every face split, tests/golden/split_482_pole.npz `all`), jittered copies,
the union's rows interleaved (row 16 i + m = vertex i of mesh m: as far from grouped as an order gets).  The loop is given its
best case: every mesh's maps, vertices, camera and gradient rows are contiguous tensors of their own, made once.  The two arms
alternate inside every round of one process (same machine, same clocks); per shape the table gives the median of the rounds,
each arm's own range over the rounds and whether the ragged call wins by more than that spread: median(loop) - median(ragged) >
max(range of ragged, range of loop).

profiles/ragged_pooling.txt holds the kernels' resource figures (tools/kernel_resources.sh) followed by this tool's output: with
--out FILE the tool keeps whatever stands in FILE in front of the line that starts with MARKER and replaces the rest.

    python tools/time_ragged_pooling.py [--rounds 7] [--seconds 0.6] [--out FILE]
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
from geometrics_amd import meshgen, utils

GOLDEN = os.path.join(ROOT, "tests", "golden")
B = 16
CHANNELS, DIMS = (64, 128, 256, 512), (56, 28, 14, 7)
MARKER = "# ---- timing"


def shapes():
    yield "482 unsplit", np.load(os.path.join(GOLDEN, "adj_482.npz"))["verts"]
    yield "1442 split", np.load(os.path.join(GOLDEN, "split_482_pole.npz"))["all.verts"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.6, help="timed work per arm and shape, over all rounds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gpu = torch.device("cuda:0")
    lines = [MARKER + ": image-feature pooling of %d meshes with their own vertices, forward + backward (maps and positions), eager,"
             % B, "# microseconds per batch; %s; maps %s x %s; rounds = %d, arms alternating, >= %.1f s of timed work per arm"
             % (torch.cuda.get_device_name(gpu), CHANNELS, DIMS, args.rounds, args.seconds),
             "# ragged = ONE utils.ragged_pooling call on the union (rows interleaved); loop = %d utils.batched_pooling calls at b = 1" % B,
             "# medians over the rounds; range = max - min of an arm's rounds; ratio = median loop / median ragged;",
             "# 'wins' = median loop - median ragged > max(range ragged, range loop)",
             "%-12s %7s %7s %10s %10s %10s %10s %7s %5s" % ("shape", "verts", "union", "ragged us", "range", "loop us", "range", "ratio", "wins")]
    bench.settle_clocks(gpu, 200)
    gen = torch.Generator().manual_seed(41)
    maps = [torch.randn(B, c, d, d, generator=gen).to(gpu) for c, d in zip(CHANNELS, DIMS)]
    img_info = torch.stack([torch.tensor([20.0 * m + 5.0, 25.0 - 3.0 * m, 1.0 + 0.02 * m]) for m in range(B)]).to(gpu)
    cam_mat, cam_pos = utils.batch_camera_info(img_info)
    for name, verts in shapes():
        nv = verts.shape[0]
        copies = torch.from_numpy(meshgen.jittered_batch(verts.astype(np.float32), B)).to(gpu)         # [B, nv, 3]
        grad = torch.randn(B, nv, sum(CHANNELS), generator=gen).to(gpu)
        union = copies.transpose(0, 1).reshape(-1, 3).clone().requires_grad_(True)                       # row 16 i + m
        union_grad = grad.transpose(0, 1).reshape(B * nv, -1).contiguous()
        vert_mesh = torch.arange(B, device=gpu, dtype=torch.int32).repeat(nv)
        union_maps = [t.clone().requires_grad_(True) for t in maps]
        singles = [(copies[m:m + 1].clone().requires_grad_(True), [t[m:m + 1].clone().requires_grad_(True) for t in maps],
                    (cam_mat[m:m + 1].clone(), cam_pos[m:m + 1].clone()), grad[m:m + 1].clone()) for m in range(B)]

        def ragged_step():
            union.grad = None
            for t in union_maps:
                t.grad = None
            utils.ragged_pooling(union_maps, union, vert_mesh, (cam_mat, cam_pos)).backward(union_grad)

        def loop_step():
            for v, mm, cams, g in singles:
                v.grad = None
                for t in mm:
                    t.grad = None
                utils.batched_pooling(mm, v, cams).backward(g)

        def events_us(work, count):
            work()                                                    # (warm: the arm's first call after the other's)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(count):
                work()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / count
        for work in (ragged_step, loop_step):
            for _ in range(3):
                work()
        torch.cuda.synchronize()
        # the two arms agree before they are timed: features' gradient rows of mesh 5 (the positions: bit for bit)
        assert torch.equal(union.grad.view(nv, B, 3)[:, 5], singles[5][0].grad[0])
        probe = max(events_us(ragged_step, 3), events_us(loop_step, 3))      # steps per round: --seconds of work per arm in all
        count = max(5, int(args.seconds * 1e6 / (probe * args.rounds)) + 1)
        rounds = [(events_us(ragged_step, count), events_us(loop_step, count)) for _ in range(args.rounds)]
        rs, ls = [r for r, _ in rounds], [l for _, l in rounds]
        mr, ml = statistics.median(rs), statistics.median(ls)
        rr, rl = max(rs) - min(rs), max(ls) - min(ls)
        lines.append("%-12s %7d %7d %10.1f %10.1f %10.1f %10.1f %7.3f %5s" % (name, nv, B * nv, mr, rr, ml, rl, ml / mr,
                                                                            "yes" if ml - mr > max(rr, rl) else "no"))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        front = ""
        if os.path.exists(args.out):
            with open(args.out) as f:
                front = f.read().split(MARKER)[0]
        with open(args.out, "w") as f:
            f.write(front + text)


if __name__ == "__main__":
    main()
