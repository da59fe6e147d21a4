"""Time of the centered-clipping middle step (2 L + 1 launches: init, L x (weights, step)) next to the trimmed
mean and to reduce_bcast_bf16, the single-pass kernels it stands beside in the `direct` exchange: all in one
process, calls interleaved, device events around each call, median over the repetitions. Shapes: the shard of a
GPT-2-small (124M) and of a 268M-element buffer on P = 4 and 8 peers.

    python scripts/cclip_kernel_table.py [--out profiles/cclip_reduce.txt] [--reps 30]

Needs the GPU: there is nothing to time without one.
"""
import torch

from _kernel_table import BUFFERS, parse_args, time_interleaved, write_table

from distributedvolunteercomputing_amd import ops  # noqa: E402  (_kernel_table put the repository on the path)
from distributedvolunteercomputing_amd.ops import robust  # noqa: E402

ITERS = (1, 3)


def cclip_bytes(P: int, n: int, L: int) -> int:
    """Bytes the 2 L + 1 launches have to move: every pass reads the P rows (bf16); init writes the centre (fp32),
    each step reads it and all but the last write it back; the last writes (P + 1) n bf16. The chunk partials and
    the weights kernel (4 P bytes per 4096 elements and pass) are left out."""
    return (L + 1) * P * n * 2 + n * 4 + L * n * 4 + (L - 1) * n * 4 + (P + 1) * n * 2


def main(argv=None):
    a = parse_args(__file__, __doc__, "profiles/cclip_reduce.txt", 30, argv)
    ops.native()
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median of {a.reps} calls each, interleaved, device events",
             "# out is a buffer of its own here, so the input keeps its random values from call to call",
             f"{'buffer':16s} {'P':>2s} {'n per shard':>11s} {'call':26s} {'launches':>8s} {'median us':>10s} "
             f"{'min us':>9s} {'MB moved':>9s} {'TB/s':>6s} {'vs trimmed':>10s} {'vs (L+1) trimmed':>16s}"]
    for name, total in BUFFERS:
        for P in a.peers:
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
            res = time_interleaved({k: v[0] for k, v in fns.items()}, a.reps, warmup=3)
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
    write_table(lines, a.out)


if __name__ == "__main__":
    main()
