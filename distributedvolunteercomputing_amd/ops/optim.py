"""Flat-buffer optimizer and local-SGD kernels (HIP on GPU, torch reference on CPU).

`ostate` is a 4-float device tensor {step, lr, clip_coef, grad_sumsq}; see optim.hip.
"""
from __future__ import annotations

import torch

from ._lib import native, use_native

OS_STEP, OS_LR, OS_CLIP, OS_SUMSQ = 0, 1, 2, 3


def new_ostate(device, lr: float) -> torch.Tensor:
    s = torch.zeros(4, dtype=torch.float32, device=device)
    s[OS_LR] = lr
    s[OS_CLIP] = 1.0
    return s


def adamw_step(param, grad, master, m, v, ostate, *, n_decay, beta1, beta2, eps, wd, max_norm=0.0):
    """One AdamW step on flat buffers (graph-capturable on GPU)."""
    if use_native(param):
        C = native()
        if max_norm > 0:
            ostate[OS_SUMSQ].zero_()
            C.grad_sumsq(grad, ostate)
        C.adam_prologue(ostate, float(max_norm))
        C.adamw_flat(param, grad, master, m, v, int(n_decay), ostate, beta1, beta2, eps, wd)
        return
    # ---- CPU reference (same math, fp32)
    g = grad.float()
    ostate[OS_STEP] += 1
    coef = 1.0
    if max_norm > 0:
        nrm = g.norm().item()
        coef = min(1.0, max_norm / (nrm + 1e-6))
        ostate[OS_SUMSQ] = nrm * nrm
    ostate[OS_CLIP] = coef
    step = ostate[OS_STEP].item()
    lr = ostate[OS_LR].item()
    g = g * coef
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1**step
    bc2 = 1 - beta2**step
    denom = v.sqrt() / (bc2**0.5) + eps
    if n_decay > 0:
        master[:n_decay].mul_(1 - lr * wd)
    master.addcdiv_(m, denom, value=-lr / bc1)
    param.copy_(master.to(param.dtype))


# ------------------------------------------------------------------ compact optimizer state
# fp8 (e4m3fn) m and fp16 v with one shared power-of-two exponent per block of CS_BLOCK elements;
# 7.06 B/param with the fp32 master instead of 12. Format and kernels: optim.hip. The functions below
# are the torch definition of the codec; the HIP kernels agree with them bit for bit.
CS_BLOCK = 32
CS_MIN_AMAX = 2.0 ** -100  # blocks below this encode as zeros with exponent byte 0
COMPACT_MAX_BETAS = (0.9, 0.999)


def check_compact_betas(betas):
    """Refuse EMA rates the compact formats cannot follow. With round-to-nearest a stored EMA stops
    moving once one step's change is under half a code step: e4m3's half step is up to 6.25 %, so m
    needs a decay of at least 10 % per step (beta1 <= 0.9); fp16's is up to 0.049 %, so v needs at
    least 0.1 % (beta2 <= 0.999)."""
    b1, b2 = float(betas[0]), float(betas[1])
    if b1 > COMPACT_MAX_BETAS[0] or b2 > COMPACT_MAX_BETAS[1]:
        raise ValueError(
            f"opt_state='compact' needs beta1 <= 0.9 and beta2 <= 0.999, got ({b1}, {b2}): with round-to-nearest "
            "an EMA held in fp8 e4m3 (half a code step up to 6.25 %) or fp16 (up to 0.049 %) stops moving when "
            "its decay per step, 1 - beta, is smaller than that; use opt_state='fp32'")


def _pow2(field: torch.Tensor) -> torch.Tensor:
    """fp32 with the biased exponent `field` (int32 in [0, 254]) and no mantissa: 2^(field - 127)."""
    return (field.to(torch.int32) << 23).view(torch.float32)


def _block_exponent(x: torch.Tensor):
    """Rows of CS_BLOCK values -> (live mask, k) with the row's amax = f 2^k, f in [0.5, 1)."""
    amax = x.abs().amax(dim=1)
    live = amax >= CS_MIN_AMAX
    _, k = torch.frexp(torch.where(live, amax, torch.ones_like(amax)))
    return live, k.to(torch.int32)


def compact_encode_m(m: torch.Tensor):
    """fp32 m[n] (n % 32 == 0, finite) -> (e4m3fn codes uint8[n], exponent bytes uint8[n / 32])."""
    x = m.reshape(-1, CS_BLOCK).float()
    live, k = _block_exponent(x)
    e = k - 8
    s = (x * _pow2(127 - e)[:, None]).clamp(-240.0, 240.0)
    code = s.to(torch.float8_e4m3fn).view(torch.uint8)
    code = torch.where(live[:, None], code, torch.zeros_like(code))
    byte = torch.where(live, e + 127, torch.zeros_like(e)).to(torch.uint8)
    return code.reshape(-1), byte


def compact_encode_v(v: torch.Tensor):
    """fp32 v[n] (non-negative, finite) -> (fp16[n], exponent bytes uint8[n / 32]). A positive element of
    a live block never encodes below the smallest fp16 subnormal, so it never decodes to 0."""
    x = v.reshape(-1, CS_BLOCK).float()
    live, k = _block_exponent(x)
    e = k - 15
    s = (x * _pow2(127 - e)[:, None]).clamp(2.0 ** -24, 32752.0)
    s = torch.where((x > 0) & live[:, None], s, torch.zeros_like(s))
    byte = torch.where(live, e + 127, torch.zeros_like(e)).to(torch.uint8)
    return s.to(torch.float16).reshape(-1), byte


def compact_decode_m(code: torch.Tensor, byte: torch.Tensor) -> torch.Tensor:
    x = code.view(torch.float8_e4m3fn).float().reshape(-1, CS_BLOCK)
    return (x * _pow2(byte)[:, None]).reshape(-1)


def compact_decode_v(half: torch.Tensor, byte: torch.Tensor) -> torch.Tensor:
    return (half.float().reshape(-1, CS_BLOCK) * _pow2(byte)[:, None]).reshape(-1)


class CompactState:
    """Adam moments of a flat range of n elements (n % 32 == 0) in the compact format: `m_code`
    uint8[n], `m_exp` uint8[n / 32], `v_half` float16[n], `v_exp` uint8[n / 32]. Non-finite moments
    (so non-finite gradients) are unsupported, as in q8."""

    FIELDS = ("m_code", "m_exp", "v_half", "v_exp")

    def __init__(self, m_code, m_exp, v_half, v_exp):
        self.m_code, self.m_exp, self.v_half, self.v_exp = m_code, m_exp, v_half, v_exp

    @classmethod
    def zeros(cls, n: int, device):
        if n % CS_BLOCK:
            raise ValueError(f"compact optimizer state needs a multiple of {CS_BLOCK} elements, got {n}")
        u8 = dict(dtype=torch.uint8, device=device)
        return cls(torch.zeros(n, **u8), torch.zeros(n // CS_BLOCK, **u8),
                   torch.zeros(n, dtype=torch.float16, device=device), torch.zeros(n // CS_BLOCK, **u8))

    @classmethod
    def from_fp32(cls, m, v):
        st = cls.zeros(m.numel(), m.device)
        st.load_fp32(m, v)
        return st

    def arrays(self):
        return self.m_code, self.m_exp, self.v_half, self.v_exp

    @property
    def numel(self) -> int:
        return self.m_code.numel()

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.arrays())

    def load_fp32(self, m, v):
        """Encode fp32 m, v into this state, in place."""
        if m.numel() != self.numel or v.numel() != self.numel:
            raise ValueError("compact optimizer state: m and v must have the state's length")
        if self.numel == 0:
            return
        if use_native(self.m_code):
            native().optstate_encode(m.float().contiguous(), v.float().contiguous(), *self.arrays())
            return
        code, mb = compact_encode_m(m)
        half, vb = compact_encode_v(v)
        for dst, src in zip(self.arrays(), (code, mb, half, vb)):
            dst.copy_(src)

    def to_fp32(self, a: int = 0, b: int | None = None):
        """(m, v) in fp32 of the elements [a, b) of this state (block-aligned; default: all)."""
        s = self if (a == 0 and b is None) else self.narrow(a, self.numel if b is None else b)
        if use_native(s.m_code) and s.numel:
            m = torch.empty(s.numel, dtype=torch.float32, device=s.m_code.device)
            v = torch.empty_like(m)
            native().optstate_decode(*s.arrays(), m, v)
            return m, v
        return compact_decode_m(s.m_code, s.m_exp), compact_decode_v(s.v_half, s.v_exp)

    def narrow(self, a: int, b: int):
        """View of the elements [a, b); a and b are multiples of the block."""
        if a % CS_BLOCK or b % CS_BLOCK or not 0 <= a <= b <= self.numel:
            raise ValueError(f"compact optimizer state: [{a}, {b}) is not a block-aligned range of {self.numel}")
        return CompactState(self.m_code[a:b], self.m_exp[a // CS_BLOCK:b // CS_BLOCK], self.v_half[a:b],
                            self.v_exp[a // CS_BLOCK:b // CS_BLOCK])

    def clone(self):
        return CompactState(*(t.clone() for t in self.arrays()))

    def copy_(self, other):
        for dst, src in zip(self.arrays(), other.arrays()):
            dst.copy_(src)
        return self

    def equal(self, other) -> bool:
        return all(torch.equal(x, y) for x, y in zip(self.arrays(), other.arrays()))


def adamw_flat_compact(param, grad, master, state: CompactState, ostate, *, n_decay, beta1, beta2, eps, wd):
    """The fused compact step alone: `ostate` already holds this step's {step, lr, clip_coef}."""
    if use_native(param):
        native().adamw_flat_compact(param, grad, master, *state.arrays(), int(n_decay), ostate, beta1, beta2, eps, wd)
        return
    st = ostate.clone()
    st[OS_STEP] -= 1  # the reference below advances the step itself
    clip = float(st[OS_CLIP])
    g = grad if clip == 1.0 else grad.float() * clip
    m, v = state.to_fp32()
    adamw_step(param, g, master, m, v, st, n_decay=n_decay, beta1=beta1, beta2=beta2, eps=eps, wd=wd, max_norm=0.0)
    state.load_fp32(m, v)


def adamw_step_compact(param, grad, master, state: CompactState, ostate, *, n_decay, beta1, beta2, eps, wd,
                       max_norm=0.0):
    """One AdamW step on flat buffers with m and v in the compact format (graph-capturable on GPU): decode,
    the arithmetic of `adamw_step`, encode. The master and the parameters are updated from this step's
    unquantised moments. Non-finite gradients are unsupported."""
    if use_native(param):
        C = native()
        if max_norm > 0:
            ostate[OS_SUMSQ].zero_()
            C.grad_sumsq(grad, ostate)
        C.adam_prologue(ostate, float(max_norm))
        C.adamw_flat_compact(param, grad, master, *state.arrays(), int(n_decay), ostate, beta1, beta2, eps, wd)
        return
    # ---- CPU reference: decode, the reference math of adamw_step, encode
    m, v = state.to_fp32()
    adamw_step(param, grad, master, m, v, ostate, n_decay=n_decay, beta1=beta1, beta2=beta2, eps=eps, wd=wd,
               max_norm=max_norm)
    state.load_fp32(m, v)


def lsgd_delta(master, anchor, delta):
    if use_native(master) and delta.dtype == torch.bfloat16:
        native().lsgd_delta(master, anchor, delta)
    else:
        delta.copy_((master - anchor).to(delta.dtype))


def lsgd_apply(avg, anchor, master, param, mom=None, *, outer_lr=1.0, mu=0.0, nesterov=False, avg_scale=1.0):
    if use_native(avg) and avg.dtype == torch.bfloat16:
        native().lsgd_apply(avg, anchor, master, param, mom, outer_lr, mu, nesterov, avg_scale)
        return
    g = -avg.float() * avg_scale
    upd = g
    if mom is not None:
        mom.mul_(mu).add_(g)
        upd = g + mu * mom if nesterov else mom
    anchor.add_(upd, alpha=-outer_lr)
    master.copy_(anchor)
    param.copy_(anchor.to(param.dtype))


def f32_to_bf16(src, dst):
    if use_native(src):
        native().f32_to_bf16(src, dst)
    else:
        dst.copy_(src.to(dst.dtype))


def axpy_bf16(src, acc, scale=1.0):
    """acc += scale * src (bf16 buffers)."""
    if use_native(src):
        native().axpy_bf16(src, acc, scale)
    else:
        acc.copy_((acc.float() + scale * src.float()).to(acc.dtype))


def reduce_bcast_bf16(inp, out, mine, P: int):
    """Direct all-reduce middle step: sum the P rows of `inp`; write the sum to every row of
    `out` (may alias `inp`: each element is read before it is written) and to `mine`."""
    if use_native(inp):
        native().reduce_bcast_bf16(inp, out, mine, P)
        return
    red = inp.view(P, -1).float().sum(0).to(inp.dtype)
    if out is not None:
        out.view(P, -1).copy_(red.unsqueeze(0).expand(P, -1))
    if mine is not None:
        mine.copy_(red)
