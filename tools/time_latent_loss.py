"""Time the latent-loss branch of the reference's training step (GEOMetrics.py:165-171) at its shape -- 16 meshes of the
482-vertex template: BatchMeshEncoder(50) forward + latent loss + backward to the positions, parameters frozen -- on the two
routes of models.BatchMeshEncoder in ONE process:

  fused     one launch per layer and direction (geometrics_amd/encoder.py, csrc/encoder_stack.hip)
  separate  one product + one aggregation per layer (the layers' own operators)

Per route: kernel launches of the forward and of the backward pass (torch.profiler's device events of one step), the eager step
(host clock over --iters steps that end in one synchronise) and the step replayed from a HIP graph (device events).  The two
routes are timed alternately, --rounds times each; the table gives the median and the range.  Both routes' latents and position
gradients are compared first.

    python tools/time_latent_loss.py [--batch 16] [--iters 200] [--rounds 5] [--out profiles/latent_loss.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geometrics_amd import encoder, meshgen, models, utils  # noqa: E402


def setup(batch, dev, seed=7):
    torch.manual_seed(seed)
    V, F = meshgen.uv_sphere()
    adj = utils.adj_init(torch.from_numpy(F).to(dev))["adj"]
    enc = models.BatchMeshEncoder(50).to(dev)          # the reference initialiser's scale
    with torch.no_grad():
        for p in enc.parameters():
            if p.dim() == 1:
                p.uniform_(-0.1, 0.1)
    enc.requires_grad_(False)                          # what INTEGRATION.md tells the driver to do
    pos = (torch.from_numpy(V).to(dev).unsqueeze(0) + 0.03 * torch.randn(batch, V.shape[0], 3, device=dev)).requires_grad_(True)
    target = torch.randn(batch, 50, device=dev)
    on = (torch.arange(batch, device=dev) % 4 != 1).float()
    return enc, pos, adj, target, on


def step(enc, pos, adj, target, on):
    lat = enc(pos, adj)
    loss = utils.latent_loss(lat, target, on)
    (grad,) = torch.autograd.grad(loss, pos)
    return lat.detach(), grad


def launches(state):
    """(forward, backward) device kernels of one step, or None where the profiler gives no device events."""
    from torch.profiler import ProfilerActivity, profile
    enc, pos, adj, target, on = state

    def count(fn):
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            out = fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return out, n
    try:
        loss, fwd = count(lambda: utils.latent_loss(enc(pos, adj), target, on))
        _, bwd = count(lambda: torch.autograd.grad(loss, pos))
    except Exception as e:      # a build of torch without device tracing
        print("profiler: %s" % e, file=sys.stderr)
        return None
    return (fwd, bwd) if fwd and bwd else None


def time_eager(state, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step(*state)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def capture(state):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*state)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(*state)
    return graph, out


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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_loss.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    state = setup(args.batch, dev)
    routes = (("fused", True), ("separate", False))
    results, graphs, counts = {}, {}, {}
    for name, on in routes:
        encoder.enabled = on
        for _ in range(3):
            results[name] = step(*state)
        assert state[0].last_route == name, (state[0].last_route, name)
        counts[name] = launches(state)
        graphs[name] = capture(state)
    lat_err = float((results["fused"][0] - results["separate"][0]).abs().max() / results["separate"][0].abs().max())
    grad_err = float((results["fused"][1] - results["separate"][1]).abs().max() / results["separate"][1].abs().max())
    eager = {name: [] for name, _ in routes}
    replay = {name: [] for name, _ in routes}
    for _ in range(args.rounds):                        # alternate: both routes see the same machine
        for name, on in routes:
            encoder.enabled = on
            eager[name].append(time_eager(state, args.iters))
            time_graph(graphs[name][0], 10)
            replay[name].append(time_graph(graphs[name][0], args.iters))
    lines = ["# tools/time_latent_loss.py --batch %d --iters %d --rounds %d on %s" % (args.batch, args.iters, args.rounds,
                                                                                      torch.cuda.get_device_name(0)),
             "# BatchMeshEncoder(50) forward + latent loss + backward to the positions, %d x 482 vertices, frozen parameters;" % args.batch,
             "# us per step: median (min .. max) of %d alternating rounds of %d steps; launches: device kernels of one step" % (args.rounds, args.iters),
             "# fused against separate: latents %.2e, position gradient %.2e of scale" % (lat_err, grad_err),
             "%-9s %16s %17s %28s %28s" % ("route", "launches forward", "launches backward", "eager us/step", "graph replay us/step")]
    for name, _ in routes:
        c = counts[name]
        def fmt(v):
            return "%.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))
        lines.append("%-9s %16s %17s %28s %28s" % (name, c[0] if c else "not measured", c[1] if c else "not measured",
                                                   fmt(eager[name]), fmt(replay[name])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
