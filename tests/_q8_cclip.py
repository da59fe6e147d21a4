"""Input families and helpers shared by the q8 centered-clipping tests (CPU definition and gfx950 kernels), on top
of tests/_q8_robust.py: records uint8 [P, rec] plus the mask of the rows that vote."""
from __future__ import annotations

import struct

import torch

from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor
from tests._q8_robust import family as _robust_family
from tests._q8_robust import scales_of, set_scales

FAMILIES = ("honest", "ties", "garbage_row", "dead_rows", "majority_bad", "far_row")
NAN = 0x7FC00000


def _bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def bad_blocks(bps: int, seed: int = 0):
    """The blocks in which the `majority_bad` rows carry NaN scales: every third one (one block of one alone)."""
    return list(range(seed % 3, bps, 3)) if bps >= 3 else [0]


def majority_rows(K: int):
    """How many rows are bad in `majority_bad`: one more than the median rule survives."""
    return (K - 1) // 2 + 1


def family(name: str, P: int, bps: int, seed: int = 0):
    """(records uint8 [P, rec] on the CPU, live_mask) of one input family.

    honest, ties, garbage_row, dead_rows   as in tests/_q8_robust.py
    majority_bad  honest rows, rows 0 .. (K-1)//2 with NaN scales in the blocks `bad_blocks`, not in the others: the
                  centre is non-finite there, the coordinates stay frozen and come out as 0, counted
    far_row       honest rows, the last row's scales times 100: an honest direction far out, whose weight lands
                  strictly between 0 and 1
    """
    if name in ("honest", "ties", "garbage_row", "dead_rows"):
        return _robust_family(name, P, bps, seed)
    rec, mask = _robust_family("honest", P, bps, seed)
    if name == "majority_bad":
        blocks = bad_blocks(bps, seed)
        for k in range(majority_rows(P)):
            sc = [_bits(x) for x in scales_of(rec)[k].tolist()]
            for b in blocks:
                sc[b] = NAN
            set_scales(rec, k, sc)
    elif name == "far_row":
        set_scales(rec, P - 1, [_bits(x) for x in (scales_of(rec)[P - 1] * 100.0).tolist()])
    else:
        raise ValueError(name)
    return rec, mask


def reference(records: torch.Tensor, mask: int, valid: int, tau: float, iters: int):
    """Quant8Compressor.reduce_cclip_reference on the records' device: (record, weights, nonfinite, info)."""
    return Quant8Compressor.reduce_cclip_reference(records.reshape(-1), records.shape[0], mask, valid, tau, iters)


def clipping_tau(records: torch.Tensor, mask: int, valid: int) -> float:
    """An absolute radius that clips about half the live rows: the first update's median distance (what the adaptive
    rule would pick), or 1.0 where that is 0 or not finite, or with one voter."""
    if bin(mask).count("1") == 1:
        return 1.0
    t = reference(records, mask, valid, 0.0, 1)[3]["tau"][0]
    return t if 0.0 < t < float("inf") else 1.0


def run_reduce_cclip(records: torch.Tensor, mask: int, valid: int, tau: float, iters: int):
    """(record uint8 [rec], weights fp32 [P], nonfinite int) of Quant8Compressor.reduce_cclip on the records'
    device: the torch definition on CPU tensors, the HIP kernels on GPU tensors."""
    P, rec = records.shape
    m = rec * 32 // 33
    comp = Quant8Compressor(m * P, records.device)
    w = torch.full((P,), -1.0, dtype=torch.float32, device=records.device)
    bad = torch.zeros(1, dtype=torch.int64, device=records.device)
    out = comp.reduce_cclip(records.reshape(-1), P, mask, valid, tau, iters, w, bad)
    return out.clone(), w, int(bad)
