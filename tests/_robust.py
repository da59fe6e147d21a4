"""Input families shared by the trimmed-mean tests (CPU reference and gfx950 kernel)."""
from __future__ import annotations

import torch

FAMILIES = ("normal", "ties", "bad_row", "dead_rows")


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def family(name: str, P: int, n: int, seed: int = 0):
    """(x [P, n] bf16 on the CPU, live_mask) of one input family.

    normal     random values, every row votes
    ties       values drawn from {-0, +0, 1, -1}: large blocks of equal values and of +-0
    bad_row    random values, one row made of NaN, -NaN, +Inf, -Inf and +-3e38
    dead_rows  random values, every second row (at least one) is dead and its storage holds NaN
    """
    g = torch.Generator().manual_seed(1000 * P + seed)
    x = torch.randn(P, n, generator=g).to(torch.bfloat16)
    mask = (1 << P) - 1
    if name == "ties":
        pool = torch.tensor([-0.0, 0.0, 1.0, -1.0]).to(torch.bfloat16)
        x = pool[torch.randint(0, 4, (P, n), generator=g)]
    elif name == "bad_row":
        pool = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38, -3e38]).to(torch.bfloat16)
        row = pool[torch.randint(0, 5, (n,), generator=g)]
        neg_nan = torch.tensor([0xFFC0 - 0x10000], dtype=torch.int16).view(torch.bfloat16)
        row = torch.where(torch.rand(n, generator=g) < 0.2, neg_nan.expand(n), row)
        x[P // 2] = row
    elif name == "dead_rows":
        dead = list(range(1, P, 2))
        for k in dead:
            x[k] = float("nan")
            mask &= ~(1 << k)
    elif name != "normal":
        raise ValueError(name)
    return x, mask
