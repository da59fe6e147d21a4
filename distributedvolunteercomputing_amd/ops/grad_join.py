"""ResNet shortcut plumbing: a residual block's shortcut gradient joins the input gradient of the block's first
1x1 convolution inside that convolution's GEMM (``linear(..., join=, deposit=)``, models/resnet.py) instead of in
a separate elementwise pass."""
from __future__ import annotations

import torch

from ._lib import native, use_native


class GradJoin:
    """Hands one extra gradient of a linear layer's input to that layer's backward, which adds it in
    its input-gradient GEMM (beta = 1) instead of autograd adding the two gradients in a separate
    elementwise pass. Made for a residual block whose input x feeds both its first 1x1 convolution
    and the identity shortcut: ``residual_tap(x, join)`` on the shortcut passes its gradient here,
    ``linear(x2d, w, join=join)`` adds it (models/resnet.py). Protocol (one backward pass at a
    time, both sides on the autograd thread): the tap's backward runs first in practice (it becomes
    ready at the block's last BatchNorm, the convolution only at the end of the branch); whichever
    side runs second sees the other's state, so the result is right in either order.

    Projection shortcuts run the other way round: the shortcut's nodes are older than conv1's, so
    conv1's backward runs first and DEPOSITS its input gradient (``linear(..., join=j, deposit=True)``
    returns None for x); the shortcut convolution then adds its own into that buffer -- with beta = 1
    at stride 1, or as a strided in-place add at stride 2 (``subsample_tap``) instead of autograd's
    zero-filled full-size slice gradient plus a full-size add."""

    def __init__(self):
        self.pending = None  # the shortcut's gradient as the [M, K] matrix of the layer input
        self.ran = False     # the layer's backward ran without it (the tap then returns its gradient)

    def take(self):
        g, self.pending = self.pending, None
        return g


class _ResidualTap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, join):
        ctx.join = join
        join.pending, join.ran = None, False
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        join, ctx.join = ctx.join, None
        if join.ran or g.dim() != 4:
            return g, None
        gh = g.permute(0, 2, 3, 1)  # the [N, H, W, C] view the 1x1 convolution's GEMM uses
        if not gh.is_contiguous():
            return g, None
        join.pending = gh.reshape(-1, gh.shape[-1])
        return None, None


def residual_tap(x: torch.Tensor, join: GradJoin) -> torch.Tensor:
    """x itself (a view), whose gradient goes to ``join`` (channels-last 4-D x) instead of autograd."""
    return _ResidualTap.apply(x, join)


class _SubsampleTap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, join, s):
        ctx.join, ctx.s = join, s
        ctx.full = (x.shape[0], x.shape[2], x.shape[3], x.shape[1])  # N, H, W, C
        join.ran = False
        xh = x.permute(0, 2, 3, 1)
        ctx.hip = _nhwc_hip_ok(xh)
        if ctx.hip:  # csrc/kernels/batchnorm.hip subsample_kernel: 16-B lanes (torch's strided copy: ~1.4 TB/s)
            return native().subsample_nhwc(xh, s)
        return xh[:, ::s, ::s, :].contiguous()

    @staticmethod
    def backward(ctx, g):
        join, ctx.join = ctx.join, None
        s, (N, H, W, C) = ctx.s, ctx.full
        base = join.take()
        if base is not None and base.is_contiguous() and base.numel() == N * H * W * C:
            full = base.view(N, H, W, C)
            # conv1's deposited input gradient: only the strided quarter moves
            if ctx.hip and g.is_contiguous() and _nhwc_hip_ok(g) and full.dtype == g.dtype:
                native().subsample_add_nhwc(full, g, s)
            else:
                full[:, ::s, ::s, :].add_(g)
        else:
            join.ran = True
            full = g.new_zeros(N, H, W, C)
            full[:, ::s, ::s, :] = g
        return full.permute(0, 3, 1, 2), None, None


def _nhwc_hip_ok(t: torch.Tensor) -> bool:
    """A contiguous NHWC bf16 GPU tensor the strided-shortcut kernels take (C % 8 == 0, 16-B aligned)."""
    return (use_native(t) and t.dtype == torch.bfloat16 and t.dim() == 4 and t.is_contiguous() and t.shape[3] % 8 == 0
            and t.data_ptr() % 16 == 0)


def subsample_tap(x: torch.Tensor, join: GradJoin, stride: int) -> torch.Tensor:
    """The contiguous [N, H/s, W/s, C] subsample of channels-last 4-D x (a stride-s 1x1 convolution's
    input); its backward adds the gradient into the input gradient conv1 deposited in ``join``."""
    return _SubsampleTap.apply(x, join, stride)
