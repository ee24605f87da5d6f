"""Dev helper: the wide first layer's input gradient dX = G . W^T on the bf16 matrix cores (dense.backward_input_split: the planes
launch + the product, as a step issues them) against the library's product and the package's fp32 matrix-core kernel, at the
training shape and the driver step's.  HIP-graph replay, HIP events, operands rotated over three buffers (tools/time_dense.py).

    python tools/time_wide_dx.py [out.txt]
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from geometrics_amd import dense, gemm_tuning
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_dense import event_time_us

dev = torch.device("cuda")
if not gemm_tuning.enable() and gemm_tuning.status == "library default (tuning file rejected)":
    gemm_tuning.tune_products([(8, 2562, 963, 192), (16, 482, 1155, 192)], dev)      # as bench.py does: the library at its best
lines = ["library selection: " + gemm_tuning.status]
for rows, cin in ((20496, 963), (7712, 1155)):
    gs = [torch.randn(rows, 192, device=dev) for _ in range(3)]
    w = torch.randn(cin, 192, device=dev) * 0.05
    planes = dense.wide_dx_planes(w)
    outs = [torch.empty(rows, cin, device=dev) for _ in range(3)]
    fl = 2.0 * rows * cin * 192
    nrb = (rows + 15) // 16
    t = {}
    t["library (tuned selection)"] = event_time_us([lambda i=i: torch.mm(gs[i], w.t(), out=outs[i]) for i in range(3)])
    t["fp32 matrix cores (dense.backward_input)"] = event_time_us([lambda i=i: dense.backward_input(gs[i], w, out=outs[i]) for i in range(3)])
    t["split bf16: planes launch + product"] = event_time_us([lambda i=i: dense.backward_input_split(gs[i], w, out=outs[i]) for i in range(3)])
    t["   of which the planes launch"] = event_time_us([lambda: dense.wide_dx_planes(w)])
    lines.append("rows %d  cin %d  (%.2f GFLOP; fp32 MFMA floor %.1f us; bf16 issue floor %.1f us: %d row-blocks x %d column tiles x 36 MFMAs x 16 "
                 "cycles over 1024 SIMDs at 2.39 GHz; %.0f MB written)"
                 % (rows, cin, fl / 1e9, fl / 157.3e6, nrb * ((cin + 15) // 16) * 36 * 16 / 1024 / 2.39e3, nrb, (cin + 15) // 16, rows * cin * 4 / 1e6))
    for name, us in t.items():
        lines.append("   %-44s %7.1f us   %6.1f TFLOP/s (fp32-equivalent)" % (name, us, fl / us / 1e6))
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("# python tools/time_wide_dx.py (graph replay of 20 launches, HIP events, best of 3, operands rotated over three buffers)\n" + text + "\n")
