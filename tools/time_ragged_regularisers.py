"""Dev helper: the stage regularisers (edge term + Laplacian difference + displacement) of a training batch of B = 16 meshes
that each own their topology -- ONE call of utils.ragged_stage_regularisers on the union mesh (one launch forward + the sum
of its partials, one launch backward) against the loop of B per-mesh utils.stage_regularisers calls at b = 1 (existing code:
the baseline) -- forward + backward, eager, between HIP events.

Shapes: the reference's 482-vertex template (tests/golden/adj_482.npz, 960 faces) and the mesh it becomes when every face is
split (tests/golden/split_482_pole.npz `all`: 1442 vertices, 2880 active faces), 16 jittered copies each.  The loop is given
its best case: the 16 meshes share one face tensor and one dense adjacency, so its per-topology tables (CSR, vertex-face
lists) are built once, which a batch of 16 different topologies would not allow.  The two arms alternate inside every round
of one process (same box, same clocks); per shape the table gives the median of the rounds, each arm's own range over the
rounds and whether the ragged call wins by more than that spread: median(loop) - median(ragged) > max(range of ragged, range
of loop).  profiles/ragged_regularisers.txt is this tool's output.

    python tools/time_ragged_regularisers.py [--rounds 7] [--seconds 0.6] [--out FILE]
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
from geometrics_amd import meshgen, ragged, utils

GOLDEN = os.path.join(ROOT, "tests", "golden")
B = 16
WEIGHTS = dict(lap_weight=300.0, move_weight=20.0, edge_weight=300.0)


def shapes():
    """(name, verts, all faces -- the adjacency's --, the faces the edge term runs on)."""
    g = np.load(os.path.join(GOLDEN, "adj_482.npz"))
    yield "482 unsplit", g["verts"], g["faces"], g["faces"]
    g = np.load(os.path.join(GOLDEN, "split_482_pole.npz"))
    active = g["all.faces"][g["all.face_list"][:, 0, 2]]
    yield "1442 split", g["all.verts"], active, active


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.6, help="timed work per arm and shape, over all rounds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gpu = torch.device("cuda:0")
    lines = ["# stage regularisers (weights %g / %g / %g) of %d meshes with their own topology, forward + backward, eager, microseconds "
             "per batch; %s;" % (WEIGHTS["lap_weight"], WEIGHTS["move_weight"], WEIGHTS["edge_weight"], B, torch.cuda.get_device_name(gpu)),
             "# rounds = %d, arms alternating, >= %.1f s of timed work per arm" % (args.rounds, args.seconds),
             "# ragged = ONE utils.ragged_stage_regularisers call on the union mesh; loop = %d utils.stage_regularisers calls at b = 1" % B,
             "# medians over the rounds; range = max - min of an arm's rounds; ratio = median loop / median ragged;",
             "# 'wins' = median loop - median ragged > max(range ragged, range loop)",
             "%-12s %7s %7s %10s %10s %10s %10s %7s %5s" % ("shape", "verts", "faces", "ragged us", "range", "loop us", "range", "ratio", "wins")]
    bench.settle_clocks(gpu, 200)
    for name, verts, adj_faces, faces in shapes():
        nv, nf = verts.shape[0], faces.shape[0]
        cur_all = torch.from_numpy(meshgen.jittered_batch(verts.astype(np.float32), B)).to(gpu)
        prev_all = torch.from_numpy(meshgen.jittered_batch(verts.astype(np.float32), B, first=B)).to(gpu)
        faces_one = torch.from_numpy(faces.astype(np.int64)).to(gpu)
        adj_one = torch.from_numpy(adj_faces.astype(np.int64)).to(gpu)
        info = {"faces": faces_one, "adj_orig": utils.calc_adj(adj_one)}
        singles = [(prev_all[m:m + 1].clone().requires_grad_(True), cur_all[m:m + 1].clone().requires_grad_(True)) for m in range(B)]
        prev = prev_all.reshape(-1, 3).clone().requires_grad_(True)
        cur = cur_all.reshape(-1, 3).clone().requires_grad_(True)
        faces_union = torch.cat([faces_one + m * nv for m in range(B)])
        face_mesh = torch.arange(B, device=gpu).repeat_interleave(nf)
        vert_mesh = torch.arange(B, device=gpu).repeat_interleave(nv)
        csr = ragged.csr_from_faces(torch.cat([adj_one + m * nv for m in range(B)]), B * nv)

        def ragged_step():
            prev.grad = cur.grad = None
            utils.ragged_stage_regularisers(prev, cur, faces_union, face_mesh, vert_mesh, csr, B, **WEIGHTS).backward()

        def loop_step():
            for p, c in singles:
                p.grad = c.grad = None
                utils.stage_regularisers(p, c, info, **WEIGHTS).backward()

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
