"""Kernel times of the compact optimizer state against the fp32 one (device events, one process):
`adamw_flat` (28 B/param) next to `adamw_flat_compact` (18.06 B/param), alternating, and the two codec
kernels `optstate_encode` / `optstate_decode` (15.06 B/param each). Median and minimum ms per launch,
the bytes each kernel has to move and the rate that makes.

    python scripts/opt_state_kernel_table.py [n] [repeats]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributedvolunteercomputing_amd import ops  # noqa: E402
from distributedvolunteercomputing_amd.ops.optim import CompactState  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16 * 4096 * 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n -= n % 64
if not torch.cuda.is_available():
    sys.exit("opt_state_kernel_table.py times GPU kernels: no GPU found")
dev = torch.device("cuda", 0)
C = ops.native()
EXP = 2 / 32  # the two exponent bytes of a 32-element block, per element
# bytes per element a kernel must move: bf16 param written, bf16 grad read, fp32 master read and written,
# then the moments read and written (fp32 m + v: 16; codes 1 + halves 2 + exponents: 3.06 each way)
BYTES = {
    "adamw_flat": ("param 2 + grad 2 + master 8 + m 8 + v 8", 28.0),
    "adamw_flat_compact": ("param 2 + grad 2 + master 8 + codes 2 + halves 4 + exponents 0.125", 18 + 2 * EXP),
    "optstate_encode": ("m 4 + v 4 + codes 1 + halves 2 + exponents 0.06", 11 + EXP),
    "optstate_decode": ("codes 1 + halves 2 + exponents 0.06 + m 4 + v 4", 11 + EXP),
}

torch.manual_seed(0)
param = torch.randn(n, device=dev).to(torch.bfloat16)
grad = (torch.randn(n, device=dev) * 0.1).to(torch.bfloat16)
master = param.float()
m = torch.randn(n, device=dev) * 0.01
v = torch.rand(n, device=dev) * 1e-4
st = CompactState.from_fp32(m, v)
ostate = ops.new_ostate(dev, 1e-4)
ostate[0] = 10.0
kw = (n - 64 * 1000, ostate, 0.9, 0.95, 1e-8, 0.1)
RUN = {
    "adamw_flat": lambda: C.adamw_flat(param, grad, master, m, v, *kw),
    "adamw_flat_compact": lambda: C.adamw_flat_compact(param, grad, master, *st.arrays(), *kw),
    "optstate_encode": lambda: C.optstate_encode(m, v, *st.arrays()),
    "optstate_decode": lambda: C.optstate_decode(*st.arrays(), m, v),
}
ms = {k: [] for k in RUN}
for it in range(reps + 3):  # the kernels alternate; the first 3 rounds warm up
    for k, f in RUN.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        f()
        t1.record()
        t1.synchronize()
        if it >= 3:
            ms[k].append(t0.elapsed_time(t1))
print(f"n = {n} elements, {reps} launches each, alternating")
print(f"{'kernel':20s} {'median ms':>10s} {'min ms':>9s} {'GB moved':>9s} {'TB/s':>6s}  bytes per element")
for k, (what, b) in BYTES.items():
    med = statistics.median(ms[k])
    print(f"{k:20s} {med:10.3f} {min(ms[k]):9.3f} {b * n / 1e9:9.2f} {b * n / med / 1e9:6.2f}  {what}")
ratio = statistics.median(ms["adamw_flat_compact"]) / statistics.median(ms["adamw_flat"])
print(f"compact step / fp32 step = {ratio:.3f} of the time (the bytes predict {BYTES['adamw_flat_compact'][1] / 28:.3f})")
