"""Dev helper: one MeshDeformationBlock(3 + 192 + 960) forward + backward -- the BatchNorm-free block the old driver runs on one
unbatched mesh between two face splits -- on the launches per hidden layer and direction (deform.plain = True:
geom_deform_plain_{fwd,bwd}_f32, 13 + 13 launches) against the separate operators (deform.enabled = False: product and
aggregation per layer, torch's residual average), eager between HIP events, and as a HIP graph for information.

Shapes: the 482-vertex UV sphere, and the 1442-vertex mesh tests/golden/split_482_pole.npz stores after splitting every face
(`all`: table width 16, rows up to 65).  The two routes alternate inside every round of one process (same box, same clocks);
every route is timed for at least --seconds in all.  Per shape the table gives the median of the rounds, each route's own range
over the rounds (the run-to-run spread) and whether the fused route wins by more than that spread:
median(separate) - median(fused) > max(range of fused, range of separate).  profiles/plain_block.txt is this tool's output; the
route's default (deform.plain) follows its `wins` column: on only if it says yes at BOTH shapes in the eager mode.

    python tools/time_plain_block.py [--rounds 7] [--seconds 1.2] [--out FILE]
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
from geometrics_amd import deform, meshgen, models, utils


def split_all_adjacency():
    g = np.load(os.path.join(ROOT, "tests", "golden", "split_482_pole.npz"))
    nv = int(g["all.nv"])
    adj = np.zeros((nv, nv), np.float32)
    adj[g["all.adj.rows"].astype(np.int64), g["all.adj.cols"].astype(np.int64)] = g["all.adj.vals"]
    return torch.from_numpy(adj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.2, help="timed work per route, shape and mode, over all rounds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gpu = torch.device("cuda:0")
    _, faces = meshgen.uv_sphere()
    shapes = [("sphere 482", utils.adj_init(torch.from_numpy(faces).to(gpu))["adj"]), ("split 1442", split_all_adjacency().to(gpu))]
    lines = ["# one MeshDeformationBlock(3 + 192 + 960) forward + backward on ONE mesh, microseconds; %s; rounds = %d, routes "
             "alternating, >= %.1f s of timed work per route" % (torch.cuda.get_device_name(gpu), args.rounds, args.seconds),
             "# fused = geom_deform_plain_{fwd,bwd}_f32 (13 + 13 launches); separate = deform.enabled False (product + aggregation per layer)",
             "# medians over the rounds; range = max - min of a route's rounds; ratio = median separate / median fused;",
             "# 'wins' = median separate - median fused > max(range fused, range separate)",
             "%-11s %6s %10s %10s %12s %10s %7s %5s" % ("shape", "mode", "fused us", "range", "separate us", "range", "ratio", "wins")]
    torch.manual_seed(0)
    block = models.MeshDeformationBlock(3 + 192 + 960).to(gpu).train()
    params = list(block.parameters())
    bench.settle_clocks(gpu, 200)
    deform.plain = True
    for name, adj in shapes:
        nv = adj.shape[0]
        feats = torch.randn(nv, 3 + 192, device=gpu, requires_grad=True)
        pooled = torch.randn(nv, 960, device=gpu, requires_grad=True)
        g_f, g_c = torch.randn(nv, 192, device=gpu), torch.randn(nv, 3, device=gpu)

        def step():
            for p in params:
                p.grad = None
            feats.grad = pooled.grad = None
            f, c = block(feats, pooled, adj)
            ((f * g_f).sum() + (c * g_c).sum()).backward()
        side = torch.cuda.Stream()
        graphs = {}
        for route in (True, False):
            deform.enabled = route
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graphs[route] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[route], stream=side, capture_error_mode="thread_local"):
                step()

        def events_us(work, count):
            work()                                                    # (warm: the route's first call after the other's)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(count):
                work()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / count

        def eager(route, count):
            deform.enabled = route
            return events_us(step, count)

        def graph(route, count):
            return events_us(graphs[route].replay, count)
        for mode, fn in (("eager", eager), ("graph", graph)):
            probe = max(fn(True, 5), fn(False, 5))                     # steps per round: --seconds of work per route in all
            count = max(10, int(args.seconds * 1e6 / (probe * args.rounds)) + 1)
            rounds = [(fn(True, count), fn(False, count)) for _ in range(args.rounds)]
            fs, ss = [f for f, _ in rounds], [s for _, s in rounds]
            mf, ms = statistics.median(fs), statistics.median(ss)
            rf, rs = max(fs) - min(fs), max(ss) - min(ss)
            lines.append("%-11s %6s %10.1f %10.1f %12.1f %10.1f %7.3f %5s" % (
                name, mode, mf, rf, ms, rs, ms / mf, "yes" if ms - mf > max(rf, rs) else "no"))
            print(lines[-1], flush=True)
        deform.enabled = True
        del graphs
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
