"""Time per launch of the trimmed-mean kernel next to reduce_bcast_bf16 (the sum it replaces, which
moves the same bytes): both in one process, launches interleaved, device events around each launch,
median over the repetitions. Shapes: the shard of a GPT-2-small (124M) and of a 268M-element buffer
on P = 4 and 8 peers.

    python scripts/robust_kernel_table.py [--out profiles/robust_reduce.txt] [--reps 40]

Needs the GPU: there is nothing to time without one.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from distributedvolunteercomputing_amd import ops  # noqa: E402

BUFFERS = (("gpt2-small 124M", 124_439_808), ("268M", 268_435_456))
PEERS = (4, 8)


def _time(fn, reps, warmup=5):
    """Median / min ms per launch of each fn in `fn` (a dict), launches interleaved."""
    for _ in range(warmup):
        for f in fn.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fn}
    for _ in range(reps):
        for k, f in fn.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    return {k: (statistics.median(v), min(v)) for k, v in ms.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/robust_reduce.txt")
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("robust_kernel_table: no GPU, nothing measured")
    ops.native()
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median of {a.reps} launches each, interleaved, device events",
             "# bytes moved per launch: P n read + (P + 1) n written, bf16 (out is a buffer of its own here, so the",
             "# input keeps its random values from launch to launch; the collective aliases it onto the input)",
             f"{'buffer':16s} {'P':>2s} {'n per shard':>11s} {'kernel':28s} {'median us':>10s} {'min us':>9s} "
             f"{'MB moved':>9s} {'TB/s':>6s} {'vs sum':>7s}"]
    for name, total in BUFFERS:
        for P in PEERS:
            n = total // P // 8 * 8
            g = torch.Generator(device=dev).manual_seed(P)
            inp = (0.01 * torch.randn(P * n, device=dev, generator=g)).to(torch.bfloat16)
            out = torch.empty_like(inp)
            mine = torch.empty(n, dtype=torch.bfloat16, device=dev)
            counts = torch.zeros(P, dtype=torch.int64, device=dev)
            fns = {
                "reduce_bcast_bf16 (sum)": lambda: ops.reduce_bcast_bf16(inp, out, mine, P),
                "trimmed trim=1": lambda: ops.trimmed_reduce_bcast_bf16(inp, out, mine, P, 1, None, counts),
                "trimmed median": lambda: ops.trimmed_reduce_bcast_bf16(inp, out, mine, P, (P - 1) // 2, None, counts),
                "trimmed trim=1, no counts": lambda: ops.trimmed_reduce_bcast_bf16(inp, out, mine, P, 1, None, None),
            }
            res = _time(fns, a.reps)
            moved = (2 * P + 1) * n * 2
            base = res["reduce_bcast_bf16 (sum)"][0]
            for k, (med, mn) in res.items():
                lines.append(f"{name:16s} {P:2d} {n:11d} {k:28s} {med * 1e3:10.1f} {mn * 1e3:9.1f} {moved / 1e6:9.1f} "
                             f"{moved / (med * 1e-3) / 1e12:6.2f} {med / base:7.2f}")
            del inp, out, mine
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
