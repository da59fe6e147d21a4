"""Shared helpers of the q8 (8-bit block quantisation) tests: input families, the unpacked view of
wire records and a one-process simulation of a P-peer round (records shuffled by hand)."""
from __future__ import annotations

import torch

BLOCK = 128
HALF = 0.5 + 2.0 ** -16  # half a code unit plus the fp32 roundings of v * inv and scale (~127 * 2^-24)
TINY = 2.0 ** -100  # blocks whose maximum magnitude is below this send nothing


def families(n: int, seed: int = 0) -> dict:
    """The input families of the codec tests, fp32 [n] each (CPU)."""
    g = torch.Generator().manual_seed(seed)

    def randn():
        return torch.randn(n, generator=g)

    out = {"randn": randn(), "wide": randn() * torch.exp(8 * randn()), "1e-30": 1e-30 * randn(),
           "zeros": torch.zeros(n)}
    for lane in (0, 127):
        v = torch.zeros(n)
        v[lane::BLOCK] = randn()[lane::BLOCK]  # one non-zero per block (none where the lane is past n)
        out[f"lane{lane}"] = v
    tiny = randn() * 2.0 ** -104  # every value below 2^-100 ...
    tiny[BLOCK:2 * BLOCK] = randn()[BLOCK:2 * BLOCK]  # ... but the second block (where there is one)
    out["tiny"] = tiny
    return out


def unpack(records: torch.Tensor, P: int):
    """records uint8 [P * record] -> (codes int8 [L], scales fp32 [L / 128])."""
    w = records.view(P, -1)
    m = w.shape[1] * 32 // 33
    return w[:, :m].contiguous().view(torch.int8).view(-1), w[:, m:].contiguous().view(torch.float32).view(-1)


def simulate_round(comps, gs):
    """One averaging round of P = len(comps) peers in one process: encode on every peer, the
    all-to-all and the all-gather by torch copies. Returns (outs [P] bf16 clones, wires [P] clones,
    gathered records)."""
    P = len(comps)
    wires = [c.encode(g, P).clone() for c, g in zip(comps, gs)]
    if P == 1:
        return [comps[0].decode(wires[0], 1).clone()], wires, wires[0]
    rec = comps[0].layout(P)[2]
    records = []
    for j, c in enumerate(comps):
        recv = torch.cat([w[j * rec:(j + 1) * rec] for w in wires])
        records.append(c.reduce(recv, P).clone())
    gathered = torch.cat(records)
    return [c.decode(gathered, P).clone() for c in comps], wires, gathered
