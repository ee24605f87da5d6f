"""Time the reference driver's validation forward (GEOMetrics.py:205-224): three poolings and the blocks 963 / 1155 / 1155
-> 192 x 13 -> 3 in eval() under no_grad on the 482-vertex template, at the given batch sizes, in two forms:

  eager  wall clock over --iters forwards that end in one synchronise (what the unmodified driver gets)
  graph  the forward captured once into a HIP graph, --iters replays bracketed by device events

One JSON line per (batch, form): {"batch", "form", "us": per forward, "iters"}.  Runs on any tree of the project (it uses
only what the driver calls), so the same file times a commit and its parent.

    python tools/time_eval_forward.py [--batches 1 16 40] [--iters 50]
    python tools/time_eval_forward.py --trace 1 --iters 10     # for rocprofv3 --kernel-trace: one warm-up forward, a 2 s
                                                               # gap, then --iters eager forwards (tools/eval_forward_trace.py)
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geometrics_amd import meshgen, models, utils  # noqa: E402


def setup(batch, dev, seed=5):
    torch.manual_seed(seed)
    V, F = meshgen.uv_sphere()
    adj_info = utils.adj_init(torch.from_numpy(F).to(dev))
    initial_positions = torch.from_numpy(V).to(dev)
    blocks = [models.BatchMeshDeformationBlock(c, V.shape[0]).to(dev).eval() for c in (963, 1155, 1155)]
    with torch.no_grad():                        # running statistics of a trained model, not the (0, 1) of a fresh one
        for blk in blocks:
            for i in range(1, 14):
                bn = getattr(blk, "bn%d" % i)
                bn.running_var.copy_(torch.exp(torch.empty_like(bn.running_var).uniform_(-3.0, 6.0)))
                bn.running_mean.uniform_(-5.0, 5.0)
    maps = [[torch.randn(batch, c, d, d, device=dev) for c, d in ((64, 56), (128, 28), (256, 14), (512, 7))] for _ in range(3)]
    img_info = torch.stack([torch.tensor([30.0 + 7 * i % 360, 25.0 - i % 20, 1.0 + 0.01 * (i % 10)]) for i in range(batch)]).to(dev)
    return adj_info, initial_positions, blocks, maps, img_info


def forward(adj_info, initial_positions, blocks, maps, img_info):
    """GEOMetrics.py:205-224, line for line (under no_grad, blocks in eval())."""
    batch_size = maps[0][0].shape[0]
    num_verts = initial_positions.shape[0]
    modelA, modelB, modelC = blocks
    initial_positions_batch = initial_positions.unsqueeze(0).expand(batch_size, num_verts, 3)
    vertex_features = utils.batched_pooling(maps[0], initial_positions_batch, img_info.clone())
    vertex_features, vertex_positions_1 = modelA(initial_positions_batch, vertex_features, adj_info["adj"])
    vertex_positions_1 = initial_positions_batch + vertex_positions_1
    vertex_features = torch.cat((vertex_features, utils.batched_pooling(maps[1], vertex_positions_1.clone(), img_info.clone())), dim=-1)
    vertex_features, vertex_positions_2 = modelB(vertex_positions_1.clone(), vertex_features, adj_info["adj"])
    vertex_positions_2 = vertex_positions_2 + vertex_positions_1
    vertex_features = torch.cat((vertex_features, utils.batched_pooling(maps[2], vertex_positions_2.clone(), img_info.clone())), dim=-1)
    _, vertex_positions_3 = modelC(vertex_positions_2.clone(), vertex_features, adj_info["adj"])
    return vertex_positions_3 + vertex_positions_2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 40])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--trace", type=int, default=None, help="batch: warm-up, gap, --iters eager forwards (no timing)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.trace is not None:
        state = setup(args.trace, dev)
        with torch.no_grad():
            forward(*state)
            torch.cuda.synchronize()
            time.sleep(2.0)                      # the gap the trace reader splits at
            for _ in range(args.iters):
                forward(*state)
            torch.cuda.synchronize()
        return
    for batch in args.batches:
        state = setup(batch, dev)
        with torch.no_grad():
            for _ in range(3):
                out = forward(*state)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                out = forward(*state)
            torch.cuda.synchronize()
            eager = (time.perf_counter() - t0) / args.iters * 1e6
            print(json.dumps({"batch": batch, "form": "eager", "us": round(eager, 1), "iters": args.iters}), flush=True)
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph):
                    static = forward(*state)
            torch.cuda.current_stream().wait_stream(side)
            for _ in range(3):
                graph.replay()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                graph.replay()
            end.record()
            torch.cuda.synchronize()
            print(json.dumps({"batch": batch, "form": "graph", "us": round(start.elapsed_time(end) / args.iters * 1e3, 1),
                              "iters": args.iters}), flush=True)
        del state, out, static, graph
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
