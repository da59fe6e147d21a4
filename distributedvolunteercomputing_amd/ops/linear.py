"""Linear layer whose backward computes the weight gradient on a hand-written token-split GEMM.

The weight gradient of a token-major linear layer, dW[N, K] = dY[M, N]^T X[M, K], reduces over
all M = B*T tokens (65536 at the GPT-2 bench shape) into a small output: a single library GEMM
has only (N/256)*(K/256) output tiles (9..36 at GPT-2-small sizes) for 256 CUs and runs at
0.33-0.77 PF/s. The default is the hand-written ``gemm_wg`` (csrc/kernels/gemm_wg.hip: the token
axis split over the CUs, operands read transposed out of LDS, fp32 partials summed by a HIP kernel
directly INTO the flat gradient buffer -- ``p.grad`` is a view of it, see parallel/flat_params.py):
1.17-1.23 PF/s at the GPT-2 shapes (profiles/r5_gemm_wg.txt). The library fallback (other shapes,
``VCX_GEMM_WGRAD=lib``) splits the token axis into S chunks of ONE batched GEMM (S x more tiles in
flight; 1.3-2.3x a single GEMM, scripts/gemm_probe.py) and sums the partials the same way.

Hand-written GEMMs on the default path (round 4, profiles/r4_gemm_ps_bench.txt): the persistent
``gemm_ps`` (csrc/kernels/gemm_ps.hip, nt output stores) runs the GPT-2 MLP's fc + bias + GELU and
fc2 input gradient x gelu' + bias grad (``_MlpGelu``; 342 vs 422 us and 458 vs 541 us against the
library GEMM + pass), and the input gradients of the qkv and attention-output projections (dX = dY
W on W^T, 200 vs 207 us and 72 vs 77 us; ``dgrad_ps_ok``). The other forward GEMMs stay on the
library, where gemm_ps measures 0.86-0.97x (its stores slow the next tile's main loop:
profiles/r4_gemm_ps_diag.txt). ``VCX_GEMM=vcx`` switches the forward and input-gradient GEMMs to
the older tiled ``gemm_nt`` (csrc/kernels/gemm.hip), slower at these shapes (profiles/r2_gemm_nt.txt).
Everything else goes through ``mm``, the TunableOp-selected library GEMM (hipBLASLt / rocBLAS,
utils/tuning.py). The bias gradient is a HIP column-sum kernel added into the flat gradient buffer.

Which GEMM runs is decided in one place: ``forward_route`` (Y = X W^T + b: nt | f | narrow | lib) and
``dgrad_route`` (dX = dY W: the same three hand-written kernels on W^T, then ps | lib_nt | lib_nn), both
over ``_gemm_route``, executed by ``_gemm``. ``linear_wants_wt`` is ``dgrad_route`` asked without a
handle, and the fused MLP's GEMMs outside its two epilogue kernels are described by ``_mlp_routes``, which
``_MlpGelu`` and ``mlp_wants_wt`` both read: the model makes W^T ahead of the backward exactly where the
backward would otherwise make its own. The ``*_ok`` predicates carry the measurements behind each step of
the chain.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import config
from . import _deferred
from ._lib import grad_buffer, native, use_native
# ``linear(..., join=)`` takes a GradJoin; the taps lived here before ops/grad_join.py and stay importable from here
from .grad_join import GradJoin, residual_tap, subsample_tap  # noqa: F401

MIN_ROWS_PER_SPLIT = 2048


def set_gemm_backend(name: str):
    """'vcx' (hand-written gemm_nt where the shape tiles) or 'lib' (library GEMMs only);
    the ``gemm`` field of the runtime config (config.py)."""
    config.update(gemm="lib" if name == "lib" else "vcx")


def gemm_nt_ok(M: int, N: int, K: int, t) -> bool:
    return (config.get().gemm == "vcx" and use_native(t) and t.dtype == torch.bfloat16
            and bool(native().gemm_nt_supported(M, N, K)))


def gemm_nt(a, b, bias=None, out=None):
    """a [M, K] @ b[N, K]^T (+ bias[N]) on the hand-written MFMA kernel (caller checked gemm_nt_ok)."""
    a = a if a.stride(-1) == 1 else a.contiguous()
    out = torch.empty(a.shape[0], b.shape[0], device=a.device, dtype=a.dtype) if out is None else out
    native().gemm_nt(a, b, out, None, bias, None, 1 if bias is not None else 0)
    return out


_ZERO_BIAS: dict = {}


def narrow_gemm_ok(M: int, N: int, K: int, t) -> bool:
    """Y[M, N] = X[M, K] W[N, K]^T with a narrow output on the vision GEMM (csrc/kernels/vision.hip
    gemm_bias_act_kernel, 128 x 64/128 tiles) instead of the library: the ResNet-50 1x1 convolutions
    with 64 output channels at 56^2 (M = 401k: 21.6 vs 34.5 us, 41.8 vs 55.7, 44.1 vs 57.6) and 128 at
    the 401k-row shape (71.4 vs 75.0); at 100k rows or 256+ columns the library is faster
    (profiles/r5_resnet_1x1_probe.txt). Opt-in (config.narrow_gemm = "vision"): inside the config-3 step
    it measured even (8309 / 8293 vs 8321 / 8292 img/s), the probe's gain did not carry over."""
    return (config.get().narrow_gemm == "vision" and ((N <= 64 and M >= 131072) or (N <= 128 and M >= 393216))
            and K % 32 == 0 and use_native(t) and t.dtype == torch.bfloat16 and t.is_contiguous())


def narrow_gemm(a, w):
    """a [M, K] @ w[N, K]^T on the vision GEMM (caller checked narrow_gemm_ok)."""
    from . import vision as V

    zb = _ZERO_BIAS.get((w.shape[0], w.device))
    if zb is None:
        zb = _ZERO_BIAS[(w.shape[0], w.device)] = torch.zeros(w.shape[0], device=w.device)
    return V.gemm_bias_act(a, w.contiguous(), zb, False)


def gemm_f_ok(M: int, N: int, K: int, t) -> bool:
    """Y[M, N] = X[M, K] W[N, K]^T on the hand-written forward GEMM (csrc/kernels/gemm_f.hip) -- opt-in
    (config.gemm_fwd == "vcx"): 0.85-0.93x the library at the GPT-2 shapes (profiles/r6_gemm_f.txt)."""
    return (config.get().gemm_fwd == "vcx" and use_native(t) and t.dtype == torch.bfloat16 and t.is_contiguous()
            and bool(native().gemm_f_supported(M, N, K)))


def gemm_f(a, w, bias=None):
    """a [M, K] @ w[N, K]^T (+ bias) on gemm_f (caller checked gemm_f_ok)."""
    out = torch.empty(a.shape[0], w.shape[0], device=a.device, dtype=a.dtype)
    native().gemm_f(a, w.contiguous(), out, bias)
    return out


def transpose_weight(w):
    """W^T as a contiguous bf16 matrix (HIP transpose; weights only — a few MB)."""
    return native().transpose_bf16(w.contiguous())


def transpose_weights(ws, out=None):
    """[W^T for W in ws] (2-D bf16) in one HIP launch per ``native().JOB_TABLE_CAP`` matrices, bit-identical to
    ``transpose_weight``. ``out``: the list a previous call returned for the same weights (persistent buffers, one
    per weight), written again in place; anything else allocates. The handles are valid for the forward that made
    them and that forward's backward only: the flat AdamW kernel rewrites the weights without a version bump, so the
    caller makes them anew every forward and hands them to the ops (``linear(..., wt=)``, ``mlp_gelu(..., w1t=,
    w2t=)``) instead of caching them."""
    ws = [w.contiguous() for w in ws]
    if out is not None and not (len(out) == len(ws) and all(
            o.shape == (w.shape[1], w.shape[0]) and o.device == w.device and o.dtype == w.dtype for o, w in zip(out, ws))):
        out = None
    return native().transpose_bf16_many(ws, out)[0]


def mm(a, b, trans_a: bool = False, trans_b: bool = False, bias=None):
    """op(a) @ op(b) (+ bias) on the library (a per-shape choice between it and an in-process hipBLASLt search
    showed no in-step gain, 956 vs 957 samples/s, and was removed)."""
    if trans_b and not trans_a:  # x @ W^T (+ b): the F.linear / TunableOp GemmAndBias path
        return F.linear(a, b, bias)
    y = torch.mm(a.t() if trans_a else a, b.t() if trans_b else b)
    return y if bias is None else y.add_(bias)


def gemm_choices() -> dict:
    return {}  # bench.py reports its size; the per-shape selection it listed is gone


# ---------------------------------------------------------------- which GEMM runs
def _gemm_route(M: int, N: int, K: int, t, bias=None):
    """The hand-written kernel for out[M, N] = a[M, K] b[N, K]^T (+ bias): 'nt', 'f', 'narrow', or None."""
    if gemm_nt_ok(M, N, K, t):
        return "nt"
    if gemm_f_ok(M, N, K, t) and (bias is None or bias.is_contiguous()):
        return "f"
    if bias is None and narrow_gemm_ok(M, N, K, t):
        return "narrow"
    return None


def forward_route(M: int, N: int, K: int, t, bias=None) -> str:
    """What computes Y[M, N] = X[M, K] W[N, K]^T (+ bias): 'nt' | 'f' | 'narrow' | 'lib' (``t``: the activations)."""
    return _gemm_route(M, N, K, t, bias) or "lib"


def dgrad_route(M: int, N: int, K: int, t, handle: bool) -> str:
    """What computes dX[M, K] = dY[M, N] W[N, K] (``t``: dY; ``handle``: the layer was given W^T): 'nt' | 'f' |
    'narrow' | 'ps' read W^T, and so does 'lib_nt'; 'lib_nn' reads W."""
    route = _gemm_route(M, K, N, t)
    if route is not None:
        return route
    if dgrad_ps_ok(M, K, N, t) and not (handle and config.get().dgrad_nt_attn):
        # the persistent hand-written GEMM on B = W^T (a few MB): faster than the library at the GPT-2 attention
        # shapes (profiles/r4_gemm_ps_bench.txt: dg_qkv, dg_proj)
        return "ps"
    # a handle and no hand-written kernel for the shape: dX = dY (W^T)^T as the NT library GEMM (the GPT-2-small LM
    # head: 3.28 ms + 0.03 ms for wte^T against 3.83 ms for the NN form, profiles/bwd_helpers_step_kernels.txt); the
    # caller decides by giving the handle
    return "lib_nt" if handle else "lib_nn"


def _gemm(route: str, a, b, bias=None):
    """a[M, K] @ b[N, K]^T (+ bias) on the back-end a route names ('lib_nn' is not of this form)."""
    if route == "nt":
        return gemm_nt(a, b, bias)
    if route == "f":
        return gemm_f(a, b, bias)
    if route == "narrow":
        return narrow_gemm(a, b)
    if route == "ps":
        out = torch.empty(a.shape[0], b.shape[0], device=a.device, dtype=a.dtype)
        native().gemm_ps(a, b, out)
        return out
    assert route in ("lib", "lib_nt"), route
    return mm(a, b, trans_b=True, bias=bias)


def linear_wants_wt(M: int, w, t) -> bool:
    """True when the backward of ``linear(x[M, K], w)`` reads W^T (``t``: the activations)."""
    N, K = _w2(w).shape
    return dgrad_route(M, N, K, t, handle=False) != "lib_nn"


def mlp_wants_wt(x, w1, w2):
    """(fc, fc2): which of W1^T, W2^T the backward of ``mlp_gelu(x, w1, b1, w2)`` reads."""
    mode = _mlp_mode(x, w1, w2)
    M = x.numel() // x.shape[-1]
    if mode is None:
        return linear_wants_wt(M, w1, x), linear_wants_wt(M, w2, x)
    # fc2's input gradient is the fused-epilogue GEMM on W2^T in either mode
    return _mlp_routes(mode, M, w2.shape[0], w1.shape[0], x, handle=True)[1] != "lib_nn", True


# Big outputs (N*K >= 16M elements) with fewer tokens than this take ONE GEMM that accumulates
# straight into the bf16 .grad (beta = 1) instead of a split-M batch + fp32 partial reduction


def _splits(M: int, N: int, K: int) -> int:
    if N * K >= 16 * 1024 * 1024:  # big outputs (LM head) already fill the GPU
        if M < config.get().wgrad_big_split_min_m:
            return 1
        s = 4
    elif M >= 262144:
        # the ResNet-50 1x1 convolutions at 56^2 (M = 401k, 64..256 x 64..256 outputs): ~6k rows per
        # split; 16 splits left 25k-row GEMMs on 64 x 16 library tiles (66-125 vs 37-82 us,
        # profiles/r5_resnet_wgrad_probe.txt)
        s = 64
    else:
        s = 16
    while s > 1 and (M % s or M // s < MIN_ROWS_PER_SPLIT):
        s //= 2
    return s


def gemm_wg_ok(M: int, N: int, K: int, t) -> bool:
    """The hand-written weight-gradient GEMM (csrc/kernels/gemm_wg.hip) takes dW[N, K] from M tokens: the
    default (config.gemm_wgrad == "vcx") wherever the output is a few dozen 256 x 256 tiles that need the
    token split -- 1.17-1.23 PF/s at the GPT-2 shapes against the library's 0.81-0.98
    (profiles/r5_gemm_wg.txt). An output of one round of tiles (129..256) runs unsplit: Llama-3-8B's q / o
    projections ([4096, 4096] from 4096 tokens) 129.7 vs 146.5 us on the library; its k / v (4 splits) and
    gate / up / down (896 tiles) lost 5-11 % and stay on the library (profiles/r6_llama_wgrad.txt). The GPT-2
    LM heads ([50304, 768 | 1024], K <= 1024) take gemm_wg with 1..4 splits (config.wgrad_wide).
    Memory: the binding allocates the fp32 split partials [splits, N, K] per call from the caching allocator --
    a transient 618 MB for the GPT-2-small LM head at 4 splits (824 MB at GPT-2-medium), a few MB elsewhere;
    under a hipGraph capture it is one fixed pool allocation."""
    cfg = config.get()
    tiles = ((N + 255) // 256) * (K // 256)
    wide = cfg.wgrad_wide and K <= 1024 and M >= 32768 and tiles > 128
    one_round = 128 < tiles <= 256 and M >= 4096
    return (cfg.gemm_wgrad == "vcx" and use_native(t) and t.dtype == torch.bfloat16
            and (tiles <= 128 or one_round or wide) and (N % 256 == 0 or wide or cfg.wgrad_ragged)
            and bool(native().gemm_wg_supported(N, K, M)))


def wgrad(dy2: torch.Tensor, x2: torch.Tensor, out: torch.Tensor | None = None, accumulate: bool = False):
    """dW = dy2^T @ x2 ([M, N], [M, K] -> [N, K]); written into / added onto `out` if given."""
    M, N = dy2.shape
    K = x2.shape[1]
    if gemm_wg_ok(M, N, K, dy2) and dy2.stride(1) == 1 and x2.stride(1) == 1 and (out is None or out.is_contiguous()):
        # hand-written transposed-read MFMA GEMM, token-split fp32 partials summed into `out`
        if out is None:
            out = torch.empty(N, K, device=dy2.device, dtype=dy2.dtype)
            accumulate = False
        native().gemm_wg(dy2, x2, out, accumulate)
        return out
    S = _splits(M, N, K)
    if S == 1 or not use_native(dy2) or (N * K) % 8:
        if out is None:
            return dy2.t().mm(x2)
        if accumulate:
            out.addmm_(dy2.t(), x2)  # one GEMM with beta = 1: no separate product tensor + add pass
        else:
            torch.mm(dy2.t(), x2, out=out)
        return out
    part = torch.bmm(dy2.view(S, M // S, N).transpose(1, 2), x2.view(S, M // S, K))  # [S, N, K]
    if out is None:
        out = torch.empty(N, K, device=dy2.device, dtype=dy2.dtype)
        accumulate = False
    native().splitk_reduce(part, out, accumulate)
    return out


def _param_grads(dy2, x2, w, bias, want_w, want_b):
    """(dw, db) to hand autograd: None where the gradient went into a preset flat .grad buffer."""
    dw = db = None
    N = w.shape[0]
    gw = grad_buffer(w) if want_w else None
    gb = grad_buffer(bias) if want_b else None
    if want_w:
        if gw is not None:
            # straight into the (flat) .grad; autograd adds nothing
            wgrad(dy2, x2, out=gw.view(N, -1), accumulate=True)
        else:
            dw = wgrad(dy2, x2).view(w.shape)
    if want_b:
        if gb is not None and (N % 8) == 0:
            native().colsum_bf16(dy2, gb)  # HIP column sums added into the flat .grad
        elif (N % 8) == 0:
            db = native().colsum_bf16(dy2)
        else:
            db = dy2.sum(0, dtype=torch.float32).to(dy2.dtype)
    return dw, db


def _w2(w):
    """The [N, K] matrix of a weight: w itself, or the [N, K] view of a 1x1 convolution's [N, K, 1, 1]."""
    return w if w.dim() == 2 else w.view(w.shape[0], -1)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, bias_grad_elsewhere=False, join=None, deposit=False, wt=None):
        # w: [N, K], or a 1x1 convolution's [N, K, 1, 1] weight itself (not a view of it: its gradient
        # then goes straight into the parameter's flat .grad, no view-backward + accumulation pass)
        ctx.save_for_backward(x, w)
        # bias_grad_elsewhere: the sole consumer of y computes the bias gradient itself (column
        # sums it already has at hand) and returns it for the same bias tensor
        ctx.has_bias = b is not None and not bias_grad_elsewhere
        ctx.bias = b
        ctx.join, ctx.deposit = join, deposit
        ctx.wt = wt  # W^T made by this forward's transpose_weights (kept for a second backward pass)
        if deposit:
            join.pending, join.ran = None, False
        x2 = x.reshape(-1, x.shape[-1])
        w = _w2(w)
        route = forward_route(x2.shape[0], w.shape[0], x2.shape[1], x2, b)
        return _gemm(route, x2, w, b).view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x, w_param = ctx.saved_tensors
        w = _w2(w_param)
        N, K = w.shape
        dy2 = dy.reshape(-1, N)
        x2 = x.reshape(-1, K)
        dy2 = dy2.contiguous()
        dx = None
        join, ctx.join = ctx.join, None
        deposit = ctx.deposit
        if deposit:  # conv1 of a projection-shortcut block: runs first, leaves dx for the shortcut
            join, depo = None, join
        base = join.take() if join is not None else None
        if join is not None and base is None:
            join.ran = True
        if ctx.needs_input_grad[0] and base is not None and base.shape == (dy2.shape[0], K) and base.is_contiguous():
            # the shortcut's gradient is the C of this GEMM (beta = 1): no separate add pass
            dx = base.addmm_(dy2, w).view(x.shape)
        elif base is not None:
            dx = (mm(dy2, w) + base).view(x.shape) if ctx.needs_input_grad[0] else None
        elif ctx.needs_input_grad[0]:
            route = dgrad_route(dy2.shape[0], N, K, dy2, handle=ctx.wt is not None)
            if route == "lib_nn":
                dx = mm(dy2, w).view(x.shape)
            else:  # every other route reads W^T: the handle, or a transpose made here
                dx = _gemm(route, dy2, transpose_weight(w) if ctx.wt is None else ctx.wt).view(x.shape)
        if deposit and dx is not None and not depo.ran and dx.is_contiguous():
            depo.pending, dx = dx.view(-1, K), None
        want_w = bool(ctx.needs_input_grad[1])
        want_b = bool(ctx.has_bias and ctx.needs_input_grad[2])
        bias, ctx.bias = ctx.bias, None
        # w_param: the gradients are formed for the parameter's own shape
        dw, db = _param_grads(dy2, x2, w_param, bias, want_w, want_b)
        return dx, dw, db, None, None, None, None


def native_linear_ok(w: torch.Tensor) -> bool:
    """True when linear(x, w, ...) runs the native autograd path (where bias_grad_elsewhere applies)."""
    return use_native(w) and w.dtype == torch.bfloat16 and torch.is_grad_enabled() and w.requires_grad


def linear(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None = None,
           bias_grad_elsewhere: bool = False, join: GradJoin | None = None, deposit: bool = False,
           wt: torch.Tensor | None = None) -> torch.Tensor:
    """y = x @ w^T (+ b), x [..., K], w [N, K] (or a 1x1 convolution's [N, K, 1, 1]). With
    bias_grad_elsewhere the backward leaves the bias gradient to y's consumer (e.g.
    ``causal_attention(qkv, bias=b)``), which must then be y's only consumer and return
    d(loss)/d(b) = column sums of dy for the same tensor. ``join``: see GradJoin (deposit = this
    layer's backward leaves its input gradient in the join for a later consumer). ``wt``: w^T from this forward's
    ``transpose_weights`` (the backward then makes none of its own)."""
    if native_linear_ok(w):
        return _Linear.apply(x, w, b, bias_grad_elsewhere, join, deposit, wt)
    assert join is None, "a GradJoin needs the native linear path (its backward consumes the joined gradient)"
    return F.linear(x, _w2(w), b)


# ---------------------------------------------------------------- fused GPT-2 MLP
def dgrad_ps_ok(M: int, N: int, K: int, t) -> bool:
    """Input gradient dX[M, N] = dY[M, K] W[K, N] on gemm_ps: where it measured faster than the
    library (K <= 2304: the qkv and attention-output projections; at K = 3072 it is 3 % slower). A layer that was
    handed W^T takes the NT library GEMM on it instead while config.dgrad_nt_attn is on (``dgrad_route``)."""
    return (config.get().dgrad_ps and K <= 2304 and use_native(t) and t.dtype == torch.bfloat16
            and t.is_contiguous() and bool(native().gemm_ps_supported(M, N, K, 0)))


def gemm_ps_ok(M: int, N: int, K: int, epi: int, t) -> bool:
    """The persistent store-overlapped GEMM (csrc/kernels/gemm_ps.hip) takes this shape/epilogue."""
    return (config.get().mlp == "fused" and use_native(t) and t.dtype == torch.bfloat16
            and bool(native().gemm_ps_supported(M, N, K, epi)))


class _MlpGelu(torch.autograd.Function):
    """y = gelu_tanh(x W1^T + b1) W2^T with the two memory-bound MLP passes folded into GEMM epilogues:
    forward  fc:  one GEMM writes pre = x W1^T + b1 AND act = gelu(pre) (no bias_gelu pass);
    backward fc2-dgrad: one GEMM writes dpre = (dy W2) * gelu'(pre) and reduces db1 = sum dpre
             in its epilogue (no bias_gelu_bwd pass, dact never hits HBM).
    ``mode`` 'ps': those two GEMMs run gemm_ps (persistent, nt stores; 0.81x and 0.85x the time of the library
    GEMM + pass, profiles/r4_gemm_ps_bench.txt) and the other two what ``_mlp_routes`` names; 'nt': all
    four run the tiled gemm_nt (VCX_GEMM=vcx)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, mode, w1t=None, w2t=None):
        C = native()
        x2 = x.reshape(-1, x.shape[-1])
        M, F_ = x2.shape[0], w1.shape[0]
        pre = torch.empty(M, F_, device=x.device, dtype=x.dtype)
        act = torch.empty_like(pre)
        if mode == "ps":
            # `pre` holds gelu'(pre) (epilogue 5): the backward needs pre only for gelu', and the forward
            # already has sigmoid(2u) (VCX_MLP_GRAD_FWD=0: store pre, gelu' in the backward's epilogue 4)
            C.gemm_ps(x2, w1, pre, act, b1, None, 5 if config.get().mlp_grad_fwd else 2)
        else:
            C.gemm_nt(x2, w1, pre, act, b1, None, 2)
        y = _gemm(_mlp_routes(mode, M, w2.shape[0], F_, act, w1t is not None)[0], act, w2)
        ctx.save_for_backward(x2, w1, b1, w2, pre, act)
        ctx.xshape = x.shape
        ctx.mode = mode
        ctx.w1t, ctx.w2t = w1t, w2t  # from this forward's transpose_weights (kept for a second backward pass)
        ctx.grad_fwd = bool(mode == "ps" and config.get().mlp_grad_fwd)
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        C = native()
        x2, w1, b1, w2, pre, act = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        M, F_ = pre.shape
        gb = grad_buffer(b1) if ctx.needs_input_grad[2] else None
        # the bias gradient's fp32 column sums: a zero-at-rest buffer per (size, device, stream) that the add into
        # the flat .grad zeroes again (no fill launch per layer), a fresh zero tensor when the sums are returned
        pool = _deferred.active() if gb is not None else None
        if pool is not None:
            # deferred: this layer's own zero-at-rest row (the shared one would mix the layers' sums); its add into
            # the flat .grad is a one-row zero_src job of the pass's column-sum finish
            cs = pool.partials((F_,), dy.device, zero=True)
        else:
            cs = _colsum_buffer(F_, dy.device) if gb is not None else torch.zeros(F_, device=dy.device, dtype=torch.float32)
        dpre = torch.empty_like(pre)
        w1t = ctx.w1t
        w2t = transpose_weight(w2) if ctx.w2t is None else ctx.w2t
        if ctx.mode == "ps":
            C.gemm_ps(dy2, w2t, dpre, pre, None, cs, 6 if ctx.grad_fwd else 4)
        else:
            C.gemm_nt(dy2, w2t, dpre, pre, None, cs, 3)
        dw2, _ = _param_grads(dy2, act, w2, None, ctx.needs_input_grad[3], False)
        dw1, _ = _param_grads(dpre, x2, w1, None, ctx.needs_input_grad[1], False)
        db1 = None
        if ctx.needs_input_grad[2]:
            if pool is not None:
                pool.register(cs, gb, accumulate=True, zero_src=True)
            elif gb is not None:
                C.add_f32_into_bf16(cs, gb, True, True)
            else:
                db1 = cs.to(b1.dtype)
        dx = None
        if ctx.needs_input_grad[0]:
            route = _mlp_routes(ctx.mode, M, w1.shape[1], F_, dpre, w1t is not None)[1]
            if route == "lib_nn":
                dx = mm(dpre, w1)
            else:
                dx = _gemm(route, dpre, transpose_weight(w1) if w1t is None else w1t)
            dx = dx.view(ctx.xshape)
        return dx, dw1, db1, dw2, None, None, None


_COLSUM = {}


def _colsum_buffer(n: int, device) -> torch.Tensor:
    """Zero-at-rest fp32 [n] on `device` for the current stream: the GEMM epilogue adds column sums into it and
    add_f32_into_bf16(..., zero_src=True) leaves it zeroed again (uses on one stream are ordered)."""
    key = (n, device, torch.cuda.current_stream(device).cuda_stream)
    buf = _COLSUM.get(key)
    if buf is None:
        buf = _COLSUM[key] = torch.zeros(n, device=device, dtype=torch.float32)
    return buf


def mlp_gelu_ok(x, w1, w2) -> bool:
    return _mlp_mode(x, w1, w2) is not None


def _mlp_mode(x, w1, w2):
    """'ps' (fused epilogues on gemm_ps), 'nt' (everything on gemm_nt) or None (library + passes)."""
    if not (native_linear_ok(w1) and x.dtype == torch.bfloat16):
        return None
    M = x.numel() // x.shape[-1]
    F_, C_ = w1.shape
    if gemm_ps_ok(M, F_, C_, 2, x) and gemm_ps_ok(M, F_, w2.shape[0], 4, x):
        return "ps"
    if (gemm_nt_ok(M, F_, C_, x) and gemm_nt_ok(M, w2.shape[0], F_, x) and gemm_nt_ok(M, C_, w2.shape[0], x)
            and gemm_nt_ok(M, F_, w2.shape[0], x)):
        return "nt"
    return None


def _mlp_routes(mode: str, M: int, N: int, F_: int, t, handle: bool):
    """(fc2 forward, fc input gradient): what computes Y[M, N] = act[M, F_] W2^T and dX[M, N] = dpre[M, F_] W1 in
    the fused MLP of ``_mlp_mode`` 'ps' or 'nt' (the names of ``forward_route`` / ``dgrad_route``; ``t``: act or
    dpre; ``handle``: W1^T was given). The fc forward and the fc2 input gradient are the mode's epilogue GEMMs."""
    if mode == "nt":
        return "nt", "nt"
    # with W1^T at hand, dX = dpre (W1^T)^T as the NT library GEMM: the fc2 forward's shape and kernel, 227.7 vs
    # 251.3 us for the NN form at the GPT-2-small step (profiles/bwd_helpers_step_kernels.txt)
    return ("f" if gemm_f_ok(M, N, F_, t) else "lib"), ("lib_nt" if handle and config.get().fc_dgrad_nt else "lib_nn")


def mlp_gelu(x, w1, b1, w2, w1t=None, w2t=None):
    """gelu_tanh(x W1^T + b1) W2^T (GPT-2 MLP without the fc2 bias, which the following fused
    add + LayerNorm applies). ``w1t`` / ``w2t``: W1^T / W2^T from this forward's ``transpose_weights``."""
    mode = _mlp_mode(x, w1, w2)
    if mode is not None:
        return _MlpGelu.apply(x, w1, b1, w2, mode, w1t, w2t)
    from .activations import bias_gelu

    return linear(bias_gelu(linear(x, w1, wt=w1t), b1), w2, wt=w2t)
