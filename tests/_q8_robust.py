"""Input families shared by the q8 trimmed-mean tests (CPU definition and gfx950 kernel): what a shard
owner may find in its receive buffer, as records uint8 [P, rec] plus the mask of the rows that vote."""
from __future__ import annotations

import struct

import torch

from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor, q8_quantise

FAMILIES = ("honest", "ties", "garbage_row", "dead_rows", "over_budget")
BLOCK = Quant8Compressor.BLOCK


# scales planted in the garbage row, as bit patterns: NaN, -NaN, +Inf, -Inf, -1.0, 3e38, a subnormal, 0
PLANTED = (0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0xBF800000, struct.unpack("<I", struct.pack("<f", 3e38))[0],
           0x00000123, 0x00000000)


def pack(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """codes int8 [bps, 128], scales fp32 [bps] -> one record uint8 [rec]."""
    return torch.cat([codes.reshape(-1).view(torch.uint8), scales.contiguous().view(torch.uint8)])


def codes_of(records: torch.Tensor) -> torch.Tensor:
    """The int8 codes [P, m] of records [P, rec] (a view)."""
    m = records.shape[1] * 32 // 33
    return records[:, :m].view(torch.int8)


def set_scales(records: torch.Tensor, row: int, patterns) -> None:
    """Overwrite the scales of one row with the given 32-bit patterns (one per block)."""
    m = records.shape[1] * 32 // 33
    b = torch.tensor([list(struct.pack("<I", p)) for p in patterns], dtype=torch.uint8).reshape(-1)
    records[row, m:] = b


def scales_of(records: torch.Tensor) -> torch.Tensor:
    """fp32 scales [P, bps] of records [P, rec] (a copy)."""
    m = records.shape[1] * 32 // 33
    return records[:, m:].contiguous().view(torch.float32)


def decoded(records: torch.Tensor) -> torch.Tensor:
    """fp32 [P, m]: float(code) * scale, the definition's decode (NaN patterns as the CPU makes them)."""
    P = records.shape[0]
    q, s = Quant8Compressor._unpack(records.reshape(-1), P)
    return (q * s).view(P, -1)


def honest(P: int, bps: int, g: torch.Generator) -> torch.Tensor:
    rows = []
    for _ in range(P):
        v = torch.randn(bps, BLOCK, generator=g) * torch.exp(4 * torch.randn(bps, BLOCK, generator=g))
        rows.append(pack(*q8_quantise(v)))
    return torch.stack(rows)


def family(name: str, P: int, bps: int, seed: int = 0, f: int = 1):
    """(records uint8 [P, rec] on the CPU, live_mask) of one input family.

    honest       encoded randn * exp(4 randn), every row votes
    ties         every peer the same record, with all-zero blocks and blocks of +-0 (a negative scale times code 0)
    garbage_row  honest rows, row P // 2 random bytes with code -128 planted and every scale of PLANTED planted in
                 a block of its own (bps >= 8; below that one of them, PLANTED[seed % 8]), the other scales random
    dead_rows    honest rows, every second row (at least one) dead and filled with 0xFF
    over_budget  honest rows, rows 0 .. f with NaN scales: one more than a trim of f takes away
    """
    g = torch.Generator().manual_seed(1000 * P + 10 * bps + seed)
    rec = honest(P, bps, g)
    mask = (1 << P) - 1
    if name == "ties":
        one = rec[0].clone().unsqueeze(0)
        c = codes_of(one).view(bps, BLOCK)
        c[::3] = 0  # all-zero blocks ...
        sc = scales_of(one)[0]
        sc[::3] = 0.0
        sc[1::3] = -sc[1::3]  # ... and blocks whose zero codes decode to -0
        c[1::3, ::2] = 0
        set_scales(one, 0, [struct.unpack("<I", struct.pack("<f", float(x)))[0] for x in sc])
        rec = one.expand(P, -1).contiguous()
    elif name == "garbage_row":
        bad = P // 2
        rec[bad] = torch.randint(0, 256, (rec.shape[1],), generator=g, dtype=torch.uint8)
        codes_of(rec)[bad, ::7] = -128
        sc = scales_of(rec)[bad].view(torch.int32).tolist()
        for i, pattern in enumerate(PLANTED if bps >= len(PLANTED) else PLANTED[seed % len(PLANTED):][:1]):
            sc[(i + seed) % bps] = pattern
        set_scales(rec, bad, [x & 0xFFFFFFFF for x in sc])
    elif name == "dead_rows":
        for k in range(1, P, 2):
            rec[k] = 0xFF
            mask &= ~(1 << k)
    elif name == "over_budget":
        for k in range(min(f + 1, P)):
            set_scales(rec, k, [0x7FC00000] * bps)
    elif name != "honest":
        raise ValueError(name)
    return rec, mask


def run_reduce_robust(records: torch.Tensor, trim: int, mask: int, valid: int):
    """(record uint8 [rec], counts [P] list, nonfinite int) of Quant8Compressor.reduce_robust on the records' device:
    the torch definition on CPU tensors, the HIP kernel on GPU tensors."""
    P, rec = records.shape
    m = rec * 32 // 33
    comp = Quant8Compressor(m * P, records.device)
    counts = torch.zeros(P, dtype=torch.int64, device=records.device)
    nonfinite = torch.zeros(1, dtype=torch.int64, device=records.device)
    out = comp.reduce_robust(records.reshape(-1), P, trim, mask, valid, counts, nonfinite)
    return out.clone(), counts.tolist(), int(nonfinite)
