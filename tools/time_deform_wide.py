"""Dev helper: one deformation block's forward + backward on the 482-vertex template at training batches above 16 meshes, the
wide launches (deform.wide = True: geom_deform_layer_wide_*, ceil(b / 16) row tiles per vertex) against the separate operators
(deform.wide = False: product, aggregation and BatchNorm as three operators each way -- from 22 meshes on torch's library
BatchNorm), eager and as a HIP graph.

The two routes alternate inside every round of one process (same box, same clocks); per batch the table gives the median of
the rounds, each route's own range over the rounds (the run-to-run spread) and whether the wide route wins by more than that
spread: median(separate) - median(wide) > max(range of wide, range of separate).  profiles/wide_batch_block.txt is this tool's
output.  A dev tool: it runs from a source checkout (it imports the checkout's bench.py for the clock conditioning).

    python tools/time_deform_wide.py [--rounds 7] [--batches 17,24,32,48,64] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from geometrics_amd import deform, meshgen, models, utils


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", default="17,24,32,48,64")
    ap.add_argument("--eager-steps", type=int, default=10)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gpu = torch.device("cuda:0")
    V, Fc = meshgen.uv_sphere()
    nv = V.shape[0]
    adj = utils.adj_init(torch.from_numpy(Fc).to(gpu))["adj"]
    lines = ["# one BatchMeshDeformationBlock(3 + 192 + 960, 482) forward + backward, microseconds; %s; rounds = %d, "
             "routes alternating" % (torch.cuda.get_device_name(gpu), args.rounds),
             "# wide = geom_deform_layer_wide_* (13 + 13 launches); separate = deform.wide False (product, aggregation, BatchNorm)",
             "# medians over the rounds; range = max - min of a route's rounds; ratio = median separate / median wide;",
             "# 'wins' = median separate - median wide > max(range wide, range separate); run from a source checkout",
             "%5s %6s %10s %10s %12s %10s %7s %5s" % ("batch", "mode", "wide us", "range", "separate us", "range", "ratio", "wins")]
    torch.manual_seed(0)
    block = models.BatchMeshDeformationBlock(3 + 192 + 960, nv).to(gpu).train()
    params = list(block.parameters())
    bench.settle_clocks(gpu, 200)
    for b in [int(x) for x in args.batches.split(",")]:
        feats = torch.randn(b, nv, 3 + 192, device=gpu, requires_grad=True)
        pooled = torch.randn(b, nv, 960, device=gpu, requires_grad=True)
        g_f, g_c = torch.randn(b, nv, 192, device=gpu), torch.randn(b, nv, 3, device=gpu)

        def step():
            for p in params:
                p.grad = None
            feats.grad = pooled.grad = None
            f, c = block(feats, pooled, adj)
            ((f * g_f).sum() + (c * g_c).sum()).backward()
        side = torch.cuda.Stream()
        graphs = {}
        for route in (True, False):
            deform.wide = route
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graphs[route] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[route], stream=side, capture_error_mode="thread_local"):
                step()

        def graph_us(route):
            g = graphs[route]
            g.replay()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.replays):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / args.replays

        def eager_us(route):
            deform.wide = route
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.eager_steps):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / args.eager_steps
        for mode, fn in (("graph", graph_us), ("eager", eager_us)):
            rounds = [(fn(True), fn(False)) for _ in range(args.rounds)]
            ws, ss = [w for w, _ in rounds], [x for _, x in rounds]
            mw, ms = statistics.median(ws), statistics.median(ss)
            rw, rs = max(ws) - min(ws), max(ss) - min(ss)
            lines.append("%5d %6s %10.1f %10.1f %12.1f %10.1f %7.3f %5s" % (
                b, mode, mw, rw, ms, rs, ms / mw, "yes" if ms - mw > max(rw, rs) else "no"))
            print(lines[-1], flush=True)
        deform.wide = True
        del graphs
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
