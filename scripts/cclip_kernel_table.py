"""Time of the centered-clipping middle step (2 L + 1 launches: init, L x (weights, step)) next to the trimmed
mean and to reduce_bcast_bf16, the single-pass kernels it stands beside in the `direct` exchange: all in one
process, calls interleaved, device events around each call, median over the repetitions. Shapes: the shard of a
GPT-2-small (124M) and of a 268M-element buffer on P = 4 and 8 peers.

    python scripts/cclip_kernel_table.py [--out profiles/cclip_reduce.txt] [--reps 30]

Needs the GPU: there is nothing to time without one.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from distributedvolunteercomputing_amd import ops  # noqa: E402
from distributedvolunteercomputing_amd.ops import robust  # noqa: E402

BUFFERS = (("gpt2-small 124M", 124_439_808), ("268M", 268_435_456))
PEERS = (4, 8)
ITERS = (1, 3)


def _time(fn, reps, warmup=3):
    """Median / min ms per call of each fn in `fn` (a dict), calls interleaved."""
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


def cclip_bytes(P: int, n: int, L: int) -> int:
    """Bytes the 2 L + 1 launches have to move: every pass reads the P rows (bf16); init writes the centre (fp32),
    each step reads it and all but the last write it back; the last writes (P + 1) n bf16. The chunk partials and
    the weights kernel (4 P bytes per 4096 elements and pass) are left out."""
    return (L + 1) * P * n * 2 + n * 4 + L * n * 4 + (L - 1) * n * 4 + (P + 1) * n * 2


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="profiles/cclip_reduce.txt")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cclip_kernel_table: no GPU, nothing measured")
    ops.native()
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median of {a.reps} calls each, interleaved, device events",
             "# out is a buffer of its own here, so the input keeps its random values from call to call",
             f"{'buffer':16s} {'P':>2s} {'n per shard':>11s} {'call':26s} {'launches':>8s} {'median us':>10s} "
             f"{'min us':>9s} {'MB moved':>9s} {'TB/s':>6s} {'vs trimmed':>10s} {'vs (L+1) trimmed':>16s}"]
    for name, total in BUFFERS:
        for P in PEERS:
            n = total // P // 8 * 8
            g = torch.Generator(device=dev).manual_seed(P)
            inp = (0.01 * torch.randn(P * n, device=dev, generator=g)).to(torch.bfloat16)
            out = torch.empty_like(inp)
            mine = torch.empty(n, dtype=torch.bfloat16, device=dev)
            w = torch.empty(P, device=dev)
            one_pass = (2 * P + 1) * n * 2
            fns = {"reduce_bcast_bf16 (sum)": (lambda: ops.reduce_bcast_bf16(inp, out, mine, P), 1, one_pass, 0),
                   "trimmed median": (lambda: ops.trimmed_reduce_bcast_bf16(inp, out, mine, P, (P - 1) // 2, None, None),
                                      1, one_pass, 0)}
            for L in ITERS:
                fns[f"cclip L={L} adaptive tau"] = (
                    lambda L=L: ops.cclip_reduce_bcast_bf16(inp, out, mine, P, 0.0, L, None, w),
                    2 * L + 1, cclip_bytes(P, n, L), L)
            res = _time({k: v[0] for k, v in fns.items()}, a.reps)
            base = res["trimmed median"][0]
            for k, (med, mn) in res.items():
                _, launches, moved, L = fns[k]
                per_pass = f"{med / ((L + 1) * base):16.2f}" if L else f"{'':16s}"
                lines.append(f"{name:16s} {P:2d} {n:11d} {k:26s} {launches:8d} {med * 1e3:10.1f} {mn * 1e3:9.1f} "
                             f"{moved / 1e6:9.1f} {moved / (med * 1e-3) / 1e12:6.2f} {med / base:10.2f} {per_pass}")
            nchunks = -(-n // robust.CCLIP_CHUNK)
            lines.append(f"# {name} P={P}: {nchunks} chunks per row; (cclip L=3 - cclip L=1) / 2 = "
                         f"{(res['cclip L=3 adaptive tau'][0] - res['cclip L=1 adaptive tau'][0]) * 500:.1f} us per "
                         f"(weights + step) pair that is not the last")
            del inp, out, mine
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
