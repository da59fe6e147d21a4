"""Coordinate-wise trimmed mean over peers (HIP on GPU bf16, torch reference otherwise).

The rule, for one element position over P rows (peers) and a bit mask `live` of the rows that vote,
K = popcount(live):

* a bf16 value with 16-bit pattern u has order key s = (u & 0x8000) ? (~u & 0xFFFF) : (u | 0x8000);
  fp32 rows use the 32-bit pattern in the same way. Ties go to the row: key = (s << 8) | row, so live
  keys are unique and the order is total: -NaN < -Inf < ... < -0 < +0 < ... < +Inf < +NaN. A
  non-finite value is always an extreme and is trimmed first.
* f = min(trim, (K - 1) // 2). Row k is kept iff it is live and its key lies between the (f+1)-th
  smallest and the (f+1)-th largest live key, inclusive: K - 2f rows. trim = 0 is the plain mean,
  trim = (K - 1) // 2 the median (for even K the mean of the two middle values).
* result = round_to_dtype((sum of the kept values) * inv): the sum in fp32, in ascending row order,
  starting from +0; inv the fp32 value of 1 / (K - 2f); no fused multiply-add. A NaN result is the
  canonical quiet NaN (0x7FC0 in bf16, 0x7FC00000 in fp32).
* counts[k] += 1 for every live row k that was not kept.

`trimmed_mean_reference` is this definition in torch; the HIP kernel (csrc/kernels/robust.hip) agrees
with it bit for bit.
"""
from __future__ import annotations

import torch

from ._lib import native, use_native

MAX_PEERS = 16  # rows the kernel sorts in registers; the pool's cap on processes per GPU node
AGGREGATES = ("mean", "trimmed", "median")


def full_mask(P: int) -> int:
    return (1 << P) - 1


def mask_of(live_ranks, P: int) -> int:
    """Bit mask of `live_ranks` (None: all P rows)."""
    if live_ranks is None:
        return full_mask(P)
    m = 0
    for r in live_ranks:
        if not 0 <= int(r) < P:
            raise ValueError(f"live rank {r} outside 0..{P - 1}")
        m |= 1 << int(r)
    return m


def effective_trim(aggregate: str, trim: int, K: int) -> int:
    """The `trim` a rule asks for among K voters, before the clip to (K - 1) // 2."""
    if aggregate == "mean":
        return 0
    if aggregate == "median":
        return (K - 1) // 2
    if aggregate == "trimmed":
        return int(trim)
    raise ValueError(f"unknown aggregation rule {aggregate!r}; choose from {AGGREGATES}")


def trim_plan(P: int, trim: int, live_mask: int):
    """(K, f, inv) of one call, after the checks every path shares."""
    if not 1 <= P <= MAX_PEERS:
        raise ValueError(f"trimmed mean: P must be in 1..{MAX_PEERS}, got {P}")
    if live_mask <= 0 or live_mask >> P:
        raise ValueError(f"trimmed mean: live_mask {live_mask:#x} must name at least one of the {P} rows and no other")
    if trim < 0:
        raise ValueError(f"trimmed mean: trim must be >= 0, got {trim}")
    K = bin(live_mask).count("1")
    f = min(int(trim), (K - 1) // 2)
    inv = float(torch.tensor(1.0 / (K - 2 * f), dtype=torch.float32))
    return K, f, inv


def order_keys(x: torch.Tensor) -> torch.Tensor:
    """int64 keys (s << 8) | row of x [P, m] (bf16 or fp32)."""
    if x.dtype == torch.bfloat16:
        u = x.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
        sign, full = 0x8000, 0xFFFF
    elif x.dtype == torch.float32:
        u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        sign, full = 0x80000000, 0xFFFFFFFF
    else:
        raise ValueError(f"trimmed mean: bf16 or fp32 rows, got {x.dtype}")
    s = torch.where((u & sign) != 0, ~u & full, u | sign)
    rows = torch.arange(x.shape[0], dtype=torch.int64, device=x.device).unsqueeze(1)
    return (s << 8) | rows


def kept_rows(x: torch.Tensor, trim: int, live_mask: int | None = None):
    """(kept, live): bool [P, m], the rows the rule keeps at every element of x [P, m], and bool [P, 1],
    the rows that vote."""
    P = x.shape[0]
    live_mask = full_mask(P) if live_mask is None else int(live_mask)
    K, f, _ = trim_plan(P, trim, live_mask)
    key = order_keys(x)
    live = torch.tensor([(live_mask >> k) & 1 == 1 for k in range(P)], device=x.device).unsqueeze(1)
    dead_key = torch.iinfo(torch.int64).max
    srt = torch.sort(torch.where(live, key, torch.full_like(key, dead_key)), dim=0).values
    lo, hi = srt[f], srt[K - 1 - f]  # the dead keys sort behind the K live ones
    return live & (key >= lo) & (key <= hi), live


def trimmed_mean_reference(x: torch.Tensor, trim: int, live_mask: int | None = None):
    """The rule of the module docstring on x [P, m] (bf16 or fp32): returns (result [m] in x's dtype,
    counts int64 [P])."""
    P = x.shape[0]
    live_mask = full_mask(P) if live_mask is None else int(live_mask)
    K, f, inv = trim_plan(P, trim, live_mask)
    kept, live = kept_rows(x, trim, live_mask)
    acc = torch.zeros(x.shape[1], dtype=torch.float32, device=x.device)
    zero = torch.zeros_like(acc)
    for k in range(P):  # ascending row order; + (+0) for a row that is not kept changes nothing
        if (live_mask >> k) & 1:
            acc = acc + torch.where(kept[k], x[k].float(), zero)
    res = acc * torch.tensor(inv, dtype=torch.float32, device=x.device)
    # the canonical NaN goes in by its bit pattern, after the rounding: torch's own fp32 -> bf16 turns a NaN
    # into 0x7FC0 or 0xFFFF depending on the code path (scalar or vectorised) that converts the element
    nan_bits = torch.tensor([0x7FC0 if x.dtype == torch.bfloat16 else 0x7FC00000], device=x.device,
                            dtype=torch.int16 if x.dtype == torch.bfloat16 else torch.int32)
    res = torch.where(torch.isnan(res), nan_bits.view(x.dtype), res.to(x.dtype))
    counts = (live & ~kept).sum(dim=1).to(torch.int64)
    return res, counts


def trimmed_reduce_bcast_bf16(inp, out, mine, P: int, trim: int, live_mask: int | None = None, counts=None):
    """Robust middle step of the direct all-reduce: the trimmed mean over the live rows of `inp` [P, n],
    written to every row of `out` (may alias `inp`, or None) and to `mine` (or None); `counts` (int64 [P],
    or None) is incremented by the trimmed elements of each live row. GPU bf16 runs the HIP kernel
    (n % 8 == 0); anything else, fp32 rows included, runs `trimmed_mean_reference`."""
    live_mask = full_mask(P) if live_mask is None else int(live_mask)
    K, f, inv = trim_plan(P, trim, live_mask)
    if inp.numel() % P:
        raise ValueError(f"trimmed mean: {inp.numel()} elements are not {P} rows")
    if use_native(inp) and inp.dtype == torch.bfloat16:
        native().trimmed_reduce_bcast_bf16(inp, out, mine, P, f, live_mask, inv, counts)
        return
    res, c = trimmed_mean_reference(inp.view(P, -1), f, live_mask)
    if out is not None:
        out.view(P, -1).copy_(res.unsqueeze(0).expand(P, -1))
    if mine is not None:
        mine.copy_(res)
    if counts is not None:
        counts.add_(c.to(counts.device))
