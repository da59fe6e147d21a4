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

Centered clipping (`cclip`; CenteredClip, Karimireddy, He, Jaggi 2021) is the per-peer rule next to it: it
bounds what one peer can do to the whole shard, in the l2 norm, where the coordinate-wise rules bound it
per coordinate. Inputs: rows x [P, m] (bf16 or fp32), the `live` mask with K voters, `tau` (fp32, finite,
>= 0; 0 = adaptive) and `iters` = L in 1..8.

1. K = 1: the result is the one live row unchanged, its weight is 1.
2. Start: v = float(trimmed_mean_reference(x, (K - 1) // 2, live)), held in fp32: the median rule's result,
   canonical NaN included. No history across rounds.
3. Distances, for l = 0 .. L-1 and every live row i: e = float(x_i[j]) - v[j] where v[j] is finite and +0
   where it is not (such a coordinate stays as it is and never votes); q = e * e, no fused multiply-add;
   D_i = sum_j q in an order that depends on m only. j is cut into chunks of 4096 elements, the ragged tail
   adds +0. In a chunk, slot t (0..255) adds its 16 values (elements 8t .. 8t+7, then 2048+8t .. 2048+8t+7)
   in ascending order from +0; the 256 slot sums are combined by the pairwise tree over adjacent indices
   with strides 1, 2, 4, ..., 128 (lower index + higher index); the chunk sums are added in ascending chunk
   order from +0.
4. Weights: d_i = sqrt(D_i), correctly rounded. A non-finite D_i gives w_i = 0, and that row is skipped, never
   multiplied. tau_l = tau if tau > 0, else the (K - 1) // 2-th smallest (0-based) of the live d_i with a
   non-finite D_i counted as +Inf. w_i = 1 if d_i <= tau_l, else tau_l / d_i (correctly rounded fp32 divide).
   Dead rows get 0.
5. Update, where v[j] is finite: v[j] += (sum over the live rows with w_i > 0, in ascending i, of
   w_i * (float(x_i[j]) - v[j])) * inv_K, inv_K the fp32 value of 1 / K; the sum starts at +0, no fused
   multiply-add.
6. Result = round_to_dtype(v) after L updates, a NaN written as the canonical quiet NaN; with it the last
   update's weights w [P] (fp32).

With an absolute tau every update moves v by at most tau in l2, so a peer moves the aggregate by at most
L * tau / K beyond the median start, whatever it sends; a peer with a non-finite value where the start is
finite has weight 0; with the adaptive tau at least (K - 1) // 2 + 1 voters have weight exactly 1, and
without an attacker the rule is close to the plain mean. `centered_clip_reference` is this definition in
torch (every add written out: torch.sum promises no order); the HIP kernels agree with it bit for bit.
"""
from __future__ import annotations

import math
import struct

import torch

from ._lib import native, use_native

MAX_PEERS = 16  # rows the kernel sorts in registers; the pool's cap on processes per GPU node
AGGREGATES = ("mean", "trimmed", "median")
AGGREGATES += ("cclip",)
CCLIP_CHUNK = 4096  # elements per chunk of a distance's summation order
CCLIP_MAX_ITERS = 8
# workgroup cap of the kernels' passes (csrc/kernels/robust.hip CC_MAX_BLOCKS): a shard of more chunks than
# this is strided over
CCLIP_MAX_WORKGROUPS = 2048


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
    if aggregate == "cclip":
        raise ValueError("cclip is no trimmed mean: it has no trim (BatchNorm buffers take the median rule under it)")
    raise ValueError(f"unknown aggregation rule {aggregate!r}; choose from {AGGREGATES}")


def _check_rows(who: str, P: int, live_mask: int):
    if not 1 <= P <= MAX_PEERS:
        raise ValueError(f"{who}: P must be in 1..{MAX_PEERS}, got {P}")
    if live_mask <= 0 or live_mask >> P:
        raise ValueError(f"{who}: live_mask {live_mask:#x} must name at least one of the {P} rows and no other")


def trim_plan(P: int, trim: int, live_mask: int):
    """(K, f, inv) of one call, after the checks every path shares."""
    _check_rows("trimmed mean", P, live_mask)
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
    counts = (live & ~kept).sum(dim=1).to(torch.int64)
    return _canonical(res, x.dtype), counts


def _write_result(res, out, mine, P: int):
    """res [n] to every row of `out` [P, n] and to `mine` [n], where they are given."""
    if out is not None:
        out.view(P, -1).copy_(res.unsqueeze(0).expand(P, -1))
    if mine is not None:
        mine.copy_(res)


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
    _write_result(res, out, mine, P)
    if counts is not None:
        counts.add_(c.to(counts.device))


# ------------------------------------------------------------------------------ centered clipping
def cclip_plan(P: int, live_mask: int, tau: float, iters: int) -> int:
    """K of one centered-clipping call, after the checks every path shares."""
    _check_rows("cclip", P, live_mask)
    check_clip(tau, iters)
    return bin(live_mask).count("1")


def check_clip(tau, iters):
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0.0 <= float(tau) <= 3.4028234663852886e38:
        raise ValueError(f"cclip: tau must be a finite fp32 number >= 0 (0: adaptive), got {tau!r}")
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= CCLIP_MAX_ITERS:
        raise ValueError(f"cclip: iters must be an integer in 1..{CCLIP_MAX_ITERS}, got {iters!r}")


def cclip_distances(x32: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """D [R] (fp32) of step 3 of the module docstring: the squared l2 distances of the rows x32 [R, m] (fp32)
    from the centre v [m] (fp32), every add in the documented order."""
    R, m = x32.shape
    zero = torch.zeros((), dtype=torch.float32, device=x32.device)
    e = torch.where(torch.isfinite(v), x32 - v, zero)
    q = e * e
    C = max(1, -(-m // CCLIP_CHUNK))
    if C * CCLIP_CHUNK != m:
        q = torch.cat([q, q.new_zeros(R, C * CCLIP_CHUNK - m)], dim=1)
    q = q.view(R, C, 2, 256, 8)
    s = q.new_zeros(R, C, 256)
    for h in range(2):  # slot t: elements 8t .. 8t+7, then 2048+8t .. 2048+8t+7, from +0
        for j in range(8):
            s = s + q[:, :, h, :, j]
    while s.shape[-1] > 1:  # the pairwise tree over adjacent indices: lower + higher
        s = s[..., 0::2] + s[..., 1::2]
    s = s[..., 0]
    D = q.new_zeros(R)
    for c in range(C):  # ascending chunk order, from +0
        D = D + s[:, c]
    return D


def _fp32(a: float) -> float:
    """The fp32 value nearest to the double a (ties to even), as a Python float."""
    return struct.unpack("f", struct.pack("f", a))[0]


def _canonical(v: torch.Tensor, dtype) -> torch.Tensor:
    """round_to_dtype(v) with a NaN written as the canonical quiet NaN."""
    # the canonical NaN goes in by its bit pattern, after the rounding: torch's own fp32 -> bf16 turns a NaN
    # into 0x7FC0 or 0xFFFF depending on the code path (scalar or vectorised) that converts the element
    nan_bits = torch.tensor([0x7FC0 if dtype == torch.bfloat16 else 0x7FC00000], device=v.device,
                            dtype=torch.int16 if dtype == torch.bfloat16 else torch.int32)
    return torch.where(torch.isnan(v), nan_bits.view(dtype), v.to(dtype))


def centered_clip_reference(x: torch.Tensor, live_mask: int | None = None, tau: float = 0.0, iters: int = 3):
    """Centered clipping of the module docstring on x [P, m] (bf16 or fp32). Returns (result [m] in x's dtype,
    w fp32 [P]: the last update's weights, info). info["tau"]: the L radii as floats; info["dist"]: L tensors
    fp32 [P] of d_i (0 for a dead row, +Inf for a non-finite D_i); info["centres"]: the L + 1 fp32 centres,
    the start first."""
    P = x.shape[0]
    live_mask = full_mask(P) if live_mask is None else int(live_mask)
    K = cclip_plan(P, live_mask, tau, iters)
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"cclip: bf16 or fp32 rows, got {x.dtype}")
    rows = [k for k in range(P) if (live_mask >> k) & 1]
    dev = x.device
    w = torch.zeros(P, dtype=torch.float32, device=dev)
    info = {"tau": [], "dist": [], "centres": []}
    if K == 1:
        w[rows[0]] = 1.0
        return x[rows[0]].clone(), w, info
    v = trimmed_mean_reference(x, (K - 1) // 2, live_mask)[0].float()
    info["centres"].append(v.clone())
    idx = torch.tensor(rows, device=dev)
    x32 = x[idx].float()  # [K, m]: the live rows, ascending
    inv_k = torch.tensor(1.0 / K, dtype=torch.float32, device=dev)
    for _ in range(iters):
        # step 4 in Python floats, whichever device holds x: torch.sqrt and the divide are not correctly rounded
        # everywhere (the GPU's are a few ulp off, the CPU's goes through a vector library and differs between
        # processors). The IEEE double square root and quotient of fp32 values, rounded to fp32, are the correctly
        # rounded fp32 results: 53 >= 2 * 24 + 2 bits, so the second rounding cannot change the outcome
        D = cclip_distances(x32, v).tolist()
        d = [_fp32(math.sqrt(a)) if math.isfinite(a) else math.inf for a in D]
        t = _fp32(tau) if tau > 0 else sorted(d)[(K - 1) // 2]
        wl = [0.0 if a == math.inf else (1.0 if a <= t else _fp32(t / a)) for a in d]
        wl = torch.tensor(wl, dtype=torch.float32, device=dev)
        d = torch.tensor(d, dtype=torch.float32, device=dev)
        acc = torch.zeros_like(v)
        for i, wi in enumerate(wl.tolist()):  # ascending row order from +0; a row with weight 0 is skipped
            if wi > 0:
                acc = acc + wl[i] * (x32[i] - v)
        v = torch.where(torch.isfinite(v), v + acc * inv_k, v)
        w = torch.zeros(P, dtype=torch.float32, device=dev).index_copy_(0, idx, wl)
        info["tau"].append(float(t))
        info["dist"].append(torch.zeros(P, dtype=torch.float32, device=dev).index_copy_(0, idx, d))
        info["centres"].append(v.clone())
    return _canonical(v, x.dtype), w, info


def cclip_reduce_bcast_bf16(inp, out, mine, P: int, tau: float, iters: int, live_mask: int | None = None,
                            weights=None):
    """Centered-clipping middle step of the direct all-reduce: the rule of the module docstring over the live
    rows of `inp` [P, n], written to every row of `out` (may alias `inp`, or None) and to `mine` (or None);
    `weights` (fp32 [P], or None) receives the last update's weights. GPU bf16 runs the HIP kernels
    (n % 8 == 0); anything else, fp32 rows included, runs `centered_clip_reference`."""
    live_mask = full_mask(P) if live_mask is None else int(live_mask)
    cclip_plan(P, live_mask, tau, iters)
    if inp.numel() % P:
        raise ValueError(f"cclip: {inp.numel()} elements are not {P} rows")
    if use_native(inp) and inp.dtype == torch.bfloat16:
        native().cclip_reduce_bcast_bf16(inp, out, mine, P, live_mask, float(tau), iters, weights)
        return
    res, w, _ = centered_clip_reference(inp.view(P, -1), live_mask, tau, iters)
    _write_result(res, out, mine, P)
    if weights is not None:
        weights.copy_(w)
