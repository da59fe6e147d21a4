"""Time of centered clipping over the q8 records (2 L + 1 launches: init, L x (weights, step)) next to
q8_trimmed_reduce on the same shard and to the bf16 centered clipping of as many elements: all in one process, calls
interleaved, device events around each call, median, min and max over the repetitions. Shapes: the shard of a
GPT-2-small (124M) and of a 268M-element buffer on P = 4 and 8 peers.

    python scripts/q8_cclip_kernel_table.py [--out profiles/q8_cclip_reduce.txt] [--reps 20]

Needs the GPU: there is nothing to time without one.
"""
import statistics

import torch

from _kernel_table import BUFFERS, parse_args, write_table

from distributedvolunteercomputing_amd import ops  # noqa: E402  (_kernel_table put the repository on the path)

ITERS = (1, 3)
BLOCK = 128


def timed(fn, reps, warmup=3):
    """(median, min, max) ms per call of each fn in `fn` (a dict), calls interleaved."""
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
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def q8_cclip_bytes(P: int, m: int, L: int) -> float:
    """(L + 1) passes of P x 1.03 + 8 bytes per element: every pass reads the P records; the fp32 centre is written
    and read once per pass, a little less in the first and the last, which write 4 and 1.03 bytes."""
    return (L + 1) * (P * (1.0 + 4.0 / BLOCK) + 8.0) * m


def main(argv=None):
    a = parse_args(__file__, __doc__, "profiles/q8_cclip_reduce.txt", 20, argv)
    C = ops.native()
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median of {a.reps} calls each, interleaved, device events",
             f"{'buffer':16s} {'P':>2s} {'m per shard':>11s} {'call':26s} {'launches':>8s} {'median us':>10s} "
             f"{'min us':>9s} {'max us':>9s} {'MB moved':>9s} {'TB/s':>6s} {'vs q8 trimmed':>13s} "
             f"{'per pass vs q8 trimmed':>22s} {'vs bf16 cclip':>13s}"]
    for name, total in BUFFERS:
        for P in a.peers:
            m = -(-total // (BLOCK * P)) * BLOCK
            rec = m + m // 32
            g = torch.Generator(device=dev).manual_seed(P)
            recv = torch.empty(P, rec, dtype=torch.uint8, device=dev)
            recv[:, :m] = torch.randint(-127, 128, (P, m), device=dev, generator=g, dtype=torch.int8).view(torch.uint8)
            scales = 1e-4 * (0.5 + torch.rand(P, m // BLOCK, device=dev, generator=g))
            recv[:, m:] = scales.view(torch.uint8)
            recv = recv.view(-1)
            out = torch.empty(rec, dtype=torch.uint8, device=dev)
            w = torch.empty(P, device=dev)
            bad = torch.zeros(1, dtype=torch.int64, device=dev)
            rows = (0.01 * torch.randn(P * m, device=dev, generator=g)).to(torch.bfloat16)
            rows_out = torch.empty_like(rows)
            mine = torch.empty(m, dtype=torch.bfloat16, device=dev)
            mask = (1 << P) - 1
            one_pass = (P + 1) * (1.0 + 4.0 / BLOCK) * m
            fns = {"q8_trimmed_reduce median": (
                lambda: C.q8_trimmed_reduce(recv, P, m, (P - 1) // 2, mask, m, out, None, bad), 1, one_pass, 0)}
            for L in ITERS:
                fns[f"cclip bf16 L={L}"] = (
                    lambda L=L: ops.cclip_reduce_bcast_bf16(rows, rows_out, mine, P, 0.0, L, None, w), 2 * L + 1,
                    float((L + 1) * P * m * 2 + m * 4 + L * m * 4 + (L - 1) * m * 4 + (P + 1) * m * 2), -L)
                fns[f"cclip q8 L={L}"] = (
                    lambda L=L: C.q8_cclip_reduce(recv, P, m, mask, m, 0.0, L, out, w, bad), 2 * L + 1,
                    q8_cclip_bytes(P, m, L), L)
            res = timed({k: v[0] for k, v in fns.items()}, a.reps)
            base = res["q8_trimmed_reduce median"][0]
            for k, (med, mn, mx) in res.items():
                _, launches, moved, L = fns[k]
                per_pass = f"{med / ((L + 1) * base):22.2f}" if L > 0 else f"{'':22s}"
                vs_bf16 = f"{med / res[f'cclip bf16 L={L}'][0]:13.2f}" if L > 0 else f"{'':13s}"
                lines.append(f"{name:16s} {P:2d} {m:11d} {k:26s} {launches:8d} {med * 1e3:10.1f} {mn * 1e3:9.1f} "
                             f"{mx * 1e3:9.1f} {moved / 1e6:9.1f} {moved / (med * 1e-3) / 1e12:6.2f} {med / base:13.2f} "
                             f"{per_pass} {vs_bf16}")
            lines.append(f"# {name} P={P}: (cclip q8 L=3 - L=1) / 2 = "
                         f"{(res['cclip q8 L=3'][0] - res['cclip q8 L=1'][0]) * 500:.1f} us per (weights + step) pair "
                         f"that is not the last")
            del recv, out, rows, rows_out, mine
    write_table(lines, a.out)


if __name__ == "__main__":
    main()
