"""Shared inputs of the compact optimizer-state tests (CPU and GPU)."""
from __future__ import annotations

import torch

from distributedvolunteercomputing_amd.ops.optim import CS_BLOCK


def adversarial(n: int, seed: int = 0):
    """fp32 (m, v) of n elements (n % 32 == 0) built to stress the codec: magnitudes spread over
    e^+-6 inside a block, exact zeros inside live blocks, all-zero blocks, blocks below the 2^-100
    cut (near 1e-37), blocks just above it, blocks near the top of the fp32 range and a block
    with a single non-zero element. Finite, v >= 0."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(n, generator=g) * torch.exp(6 * (2 * torch.rand(n, generator=g) - 1))
    v = torch.randn(n, generator=g).square() * torch.exp(6 * (2 * torch.rand(n, generator=g) - 1))
    zero = torch.rand(n, generator=g) < 0.05
    m[zero] = 0.0
    v[torch.rand(n, generator=g) < 0.05] = 0.0
    mb, vb = m.view(-1, CS_BLOCK), v.view(-1, CS_BLOCK)
    nb = mb.shape[0]
    kind = torch.arange(nb) % 16 if nb >= 16 else torch.full((nb,), -1)
    for t, scale in ((3, 0.0), (5, 1e-37), (7, 1e-29), (11, 1e30)):
        mb[kind == t] *= scale
        vb[kind == t] *= scale
    lone = kind == 13
    keep = torch.zeros(CS_BLOCK)
    keep[17] = 1.0
    mb[lone] = mb[lone] * keep + keep * 1e-3
    vb[lone] = vb[lone] * keep + keep * 1e-6
    return m, v
