"""Time optim.FusedAdam's two routes against each other in ONE process, at three tensor sets:

  bench    the 6 parameter tensors of the bench's three-layer stack
  blocks   the 168 tensors of the three deformation blocks (56 each)
  driver   a synthetic set of ~500 tensors shaped like the driver's full parameter list (the three blocks + three image
           encoders' convolution weights and biases)

  chunked  geom_adam_step_f32: up to 64 tensors per launch, lr by value (1 / 3 / 8 launches at the three sets)
  table    geom_adam_table_step_f32: one launch, per-tensor records in a device table, lr in a device array

Per set and route: the eager step() (host clock over --iters steps that end in one synchronise; gradients at stable addresses,
so the table is uploaded once) and the step replayed from a HIP graph (device events).  The two routes are timed alternately,
--rounds times each; the table gives the median and the range.  The routes' results are compared bit for bit first.

    python tools/time_adam.py [--iters 200] [--rounds 5] [--out profiles/adam_table.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geometrics_amd import optim  # noqa: E402


def block_shapes(cin):
    """The 56 parameter tensors of one deformation block: 14 layers of weight + bias and their 14 BatchNorms."""
    shapes = [(1, cin, 192), (192,)] + [(1, 192, 192), (192,)] * 12 + [(1, 192, 3), (3,)]
    return shapes + [(192,), (192,)] * 14


def encoder_shapes():
    """An image encoder of the driver's kind: 18 convolutions (3x3, 16 -> 512 channels) with bias and BatchNorm."""
    shapes, cin = [], 3
    for cout in (16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 128, 256, 256, 256, 512, 512, 512, 512):
        shapes += [(cout, cin, 3, 3), (cout,), (cout,), (cout,)]
        cin = cout
    return shapes


def tensor_sets():
    blocks = block_shapes(963) + block_shapes(1155) + block_shapes(1155)
    return (("bench", [(963, 192), (192,), (192, 192), (192,), (192, 192), (192,)]),
            ("blocks", blocks),
            ("driver", blocks + encoder_shapes() * 3 + [(512, 50), (50,)] * 60))


def make(shapes, table, seed=3):
    torch.manual_seed(seed)
    params = [torch.randn(*s, device="cuda").requires_grad_(True) for s in shapes]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-2
    return optim.FusedAdam(params, lr=1e-4, table=table)


def time_eager(opt, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def capture(opt):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    return graph


def time_graph(graph, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        graph.replay()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_table.txt"))
    args = ap.parse_args()
    routes = (("chunked", False), ("table", True))
    lines = ["# tools/time_adam.py --iters %d --rounds %d on %s" % (args.iters, args.rounds, torch.cuda.get_device_name(0)),
             "# FusedAdam.step() over the whole tensor set, gradients at stable addresses; us per step: median (min .. max) of "
             "%d alternating rounds of %d steps" % (args.rounds, args.iters),
             "%-7s %7s %10s %-8s %8s %28s %28s" % ("set", "tensors", "elements", "route", "launches", "eager us/step",
                                                    "graph replay us/step")]
    for name, shapes in tensor_sets():
        opts = {r: make(shapes, on) for r, on in routes}
        for _ in range(3):
            for opt in opts.values():
                opt.step()
        torch.cuda.synchronize()
        a, b = opts["chunked"], opts["table"]
        same = all(torch.equal(x.detach(), y.detach()) for x, y in zip(a.params + a.exp_avg + a.exp_avg_sq,
                                                                       b.params + b.exp_avg + b.exp_avg_sq))
        if not same or not torch.equal(a.state[:3], b.state[:3]):
            raise SystemExit("time_adam.py: the two routes disagree at set %r" % name)
        graphs = {r: capture(opts[r]) for r, _ in routes}
        eager = {r: [] for r, _ in routes}
        replay = {r: [] for r, _ in routes}
        for _ in range(args.rounds):                    # alternate: both routes see the same machine
            for r, _ in routes:
                eager[r].append(time_eager(opts[r], args.iters))
                time_graph(graphs[r], 10)
                replay[r].append(time_graph(graphs[r], args.iters))

        def fmt(v):
            return "%.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))
        for r, _ in routes:
            lines.append("%-7s %7d %10d %-8s %8d %28s %28s" % (name, len(shapes), sum(p.numel() for p in a.params), r,
                                                               1 if r == "table" else -(-len(shapes) // 64), fmt(eager[r]),
                                                               fmt(replay[r])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
