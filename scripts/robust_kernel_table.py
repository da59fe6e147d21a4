"""Time per launch of the trimmed-mean kernel next to reduce_bcast_bf16 (the sum it replaces, which
moves the same bytes): both in one process, launches interleaved, device events around each launch,
median over the repetitions. Shapes: the shard of a GPT-2-small (124M) and of a 268M-element buffer
on P = 4 and 8 peers.

    python scripts/robust_kernel_table.py [--out profiles/robust_reduce.txt] [--reps 40]

Needs the GPU: there is nothing to time without one.
"""
import torch

from _kernel_table import BUFFERS, parse_args, time_interleaved, write_table

from distributedvolunteercomputing_amd import ops  # noqa: E402  (_kernel_table put the repository on the path)


def main(argv=None):
    a = parse_args(__file__, __doc__, "profiles/robust_reduce.txt", 40, argv)
    ops.native()
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median of {a.reps} launches each, interleaved, device events",
             "# bytes moved per launch: P n read + (P + 1) n written, bf16 (out is a buffer of its own here, so the",
             "# input keeps its random values from launch to launch; the collective aliases it onto the input)",
             f"{'buffer':16s} {'P':>2s} {'n per shard':>11s} {'kernel':28s} {'median us':>10s} {'min us':>9s} "
             f"{'MB moved':>9s} {'TB/s':>6s} {'vs sum':>7s}"]
    for name, total in BUFFERS:
        for P in a.peers:
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
            res = time_interleaved(fns, a.reps)
            moved = (2 * P + 1) * n * 2
            base = res["reduce_bcast_bf16 (sum)"][0]
            for k, (med, mn) in res.items():
                lines.append(f"{name:16s} {P:2d} {n:11d} {k:28s} {med * 1e3:10.1f} {mn * 1e3:9.1f} {moved / 1e6:9.1f} "
                             f"{moved / (med * 1e-3) / 1e12:6.2f} {med / base:7.2f}")
            del inp, out, mine
    write_table(lines, a.out)


if __name__ == "__main__":
    main()
