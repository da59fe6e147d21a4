"""Time per launch of the q8 trimmed-mean kernel next to q8_reduce (the rank-order sum it replaces, which moves
the same bytes): both in one process, launches interleaved, device events around each launch, median over the
repetitions. Shapes: the shard of a GPT-2-small (124M) and of a 268M-element buffer on P = 4 and 8 peers.

    python scripts/q8_robust_kernel_table.py [--out profiles/q8_robust_reduce.txt] [--reps 40]

Needs the GPU: there is nothing to time without one.
"""
import torch

from _kernel_table import BUFFERS, parse_args, time_interleaved, write_table

from distributedvolunteercomputing_amd import ops  # noqa: E402  (_kernel_table put the repository on the path)
from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor  # noqa: E402


def main(argv=None):
    a = parse_args(__file__, __doc__, "profiles/q8_robust_reduce.txt", 40, argv)
    C = ops.native()
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median of {a.reps} launches each, interleaved, device events",
             "# bytes moved per launch: (P + 1) * 1.03125 B per element of the shard (P records read, one written)",
             f"{'buffer':16s} {'P':>2s} {'m per shard':>11s} {'kernel':28s} {'median us':>10s} {'min us':>9s} "
             f"{'MB moved':>9s} {'TB/s':>6s} {'vs q8_reduce':>12s}"]
    for name, total in BUFFERS:
        for P in a.peers:
            comp = Quant8Compressor(total, dev)
            L, m, rec = comp.layout(P)
            g = torch.Generator(device=dev).manual_seed(P)
            grad = (0.01 * torch.randn(total, device=dev, generator=g)).to(torch.bfloat16)
            # one peer's P wire records: honest records of P different shards, which the kernels cannot tell from
            # P peers' records of one shard
            recv = comp.encode(grad, P).clone()
            del grad, comp
            out = torch.empty(rec, dtype=torch.uint8, device=dev)
            counts = torch.zeros(P, dtype=torch.int64, device=dev)
            bad = torch.zeros(1, dtype=torch.int64, device=dev)
            mask = (1 << P) - 1
            fns = {
                "q8_reduce (sum)": lambda: C.q8_reduce(recv, P, m, 1.0 / P, out),
                "trimmed trim=1": lambda: C.q8_trimmed_reduce(recv, P, m, 1, mask, m, out, counts, bad),
                "trimmed median": lambda: C.q8_trimmed_reduce(recv, P, m, (P - 1) // 2, mask, m, out, counts, bad),
                "trimmed trim=1, no counters": lambda: C.q8_trimmed_reduce(recv, P, m, 1, mask, m, out),
            }
            res = time_interleaved(fns, a.reps)
            moved = (P + 1) * 1.03125 * m
            base = res["q8_reduce (sum)"][0]
            for k, (med, mn) in res.items():
                lines.append(f"{name:16s} {P:2d} {m:11d} {k:28s} {med * 1e3:10.1f} {mn * 1e3:9.1f} {moved / 1e6:9.1f} "
                             f"{moved / (med * 1e-3) / 1e12:6.2f} {med / base:12.2f}")
            del recv, out
    write_table(lines, a.out)


if __name__ == "__main__":
    main()
