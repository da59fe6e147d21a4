"""Per-kernel table of the q8 kernels from a rocprofv3 --kernel-trace of scripts/compress_only.py:
median time per dispatch, the bytes each kernel has to move and the rate that makes, next to the
top-k accumulate + histogram pass of the same run (the streaming yardstick of compress.hip).

    python scripts/q8_kernel_table.py <kernel_trace.csv> [n] [peers]
"""
import collections
import csv
import statistics
import sys

n = int(sys.argv[2]) if len(sys.argv) > 2 else 16 * 4096 * 4096
P = int(sys.argv[3]) if len(sys.argv) > 3 else 8
step = 128 * P
L = (n + step - 1) // step * step
m = L // P
REC = 1 + 4 / 128  # record bytes per element: one code + 1/128 of an fp32 scale
# bytes a kernel must move: bf16 g read, fp32 e read and written, records read / written
BYTES = {
    "topk_accum_hist_kernel": ("g 2 + e 4 + 4", n * (2 + 4 + 4)),
    "q8_encode_kernel": ("g 2 + e 4 + 4 + record 1.03", n * (2 + 4 + 4) + L * REC),
    "q8_reduce_kernel": (f"(P + 1) * 1.03 of the shard, P = {P}", (P + 1) * m * REC),
    "q8_decode_kernel": ("record 1.03 + out 2", L * REC + n * 2),
}
us = collections.defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    for k in BYTES:
        if k in r["Kernel_Name"]:
            us[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print(f"{'kernel':26s} {'n':>3s} {'median us':>10s} {'min us':>9s} {'MB moved':>10s} {'TB/s':>6s}  bytes per element")
for k, (what, b) in BYTES.items():
    if us[k]:
        med = statistics.median(us[k])
        print(f"{k:26s} {len(us[k]):3d} {med:10.1f} {min(us[k]):9.1f} {b / 1e6:10.1f} {b / med / 1e6:6.2f}  {what}")
