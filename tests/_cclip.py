"""Helpers shared by the centered-clipping tests (CPU reference and gfx950 kernels)."""
from __future__ import annotations

import numpy as np
import torch

from distributedvolunteercomputing_amd import ops

ATTACKS = ("none", "flip10", "x100", "nan", "ipm")


def clipping_tau(x: torch.Tensor, mask: int) -> float:
    """An absolute radius that clips about half the live rows of x: the first update's median distance
    (what the adaptive rule would pick), or 1.0 where that is 0 or not finite."""
    if bin(mask).count("1") == 1:
        return 1.0
    t = ops.centered_clip_reference(x, mask, 0.0, 1)[2]["tau"][0]
    return t if 0.0 < t < float("inf") else 1.0


def tree_distance(e: np.ndarray) -> np.float32:
    """The documented summation order of sum(e * e), written independently of ops/robust.py with numpy fp32
    scalars and vectors: chunks of 4096, 256 slots of 8 + 8 elements, the pairwise tree over adjacent slots,
    the chunk sums in ascending order."""
    e = np.asarray(e, dtype=np.float32)
    q = e * e
    m = q.size
    C = max(1, -(-m // 4096))
    q = np.concatenate([q, np.zeros(C * 4096 - m, dtype=np.float32)])
    D = np.float32(0.0)
    for c in range(C):
        ch = q[c * 4096:(c + 1) * 4096]
        s = np.zeros(256, dtype=np.float32)
        for half in (0, 2048):
            for j in range(8):
                s = s + ch[half + j:half + 2048:8]  # element half + 8 t + j of every slot t
        while s.size > 1:
            s = s[0::2] + s[1::2]
        D = np.float32(D + s[0])
    return D


def honest_rows(seed: int, K: int = 8, m: int = 8192) -> torch.Tensor:
    """K honest pseudo-gradients g + 0.3 noise (fp32)."""
    g = torch.Generator().manual_seed(seed)
    centre = torch.randn(m, generator=g)
    return centre + 0.3 * torch.randn(K, m, generator=g)


def attacked(rows: torch.Tensor, kind: str, f: int = 2):
    """(x, honest_mean, attackers): the last f rows of `rows` replaced by attackers of one kind. The honest
    mean is that of the rows left honest (in float64)."""
    if kind == "none":
        return rows.clone(), rows.double().mean(0), []
    K = rows.shape[0]
    att = list(range(K - f, K))
    hmean = rows[:K - f].double().mean(0)
    x = rows.clone()
    for k in att:
        if kind == "flip10":
            x[k] = -10.0 * rows[k]
        elif kind == "x100":
            x[k] = 100.0 * rows[k]
        elif kind == "nan":
            x[k] = float("nan")
        elif kind == "ipm":
            x[k] = (-0.5 * hmean).float()
        else:
            raise ValueError(kind)
    return x, hmean, att


def rel_l2(a: torch.Tensor, ref: torch.Tensor) -> float:
    return float((a.double() - ref.double()).norm() / ref.double().norm())
