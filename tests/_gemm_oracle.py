"""Exact-arithmetic oracle for the hand-written GEMM and implicit-GEMM convolution kernels (gemm_wg.hip,
gemm_f.hip, gemm_ps.hip, gemm.hip). Plain torch, importable without a GPU.

The idea: bf16 operands that hold small integers (times a power of two per output row / column) make every
product and every fp32 partial sum exact, whatever the accumulation order, the split count or the MFMA shape,
as long as sum |a| |b| < 2^24. The expected output is then ONE bit pattern,

    expected = (fp64 result + integer-valued bias / accumulate base).to(float32).to(bfloat16)

(the fp32 step is the kernels' `acc + bias` / `base + sum`: one fp32 addition of exact values, so it rounds the
exact sum once to fp32, and the store rounds that to bf16), and outputs are compared bit for bit. Any dropped,
duplicated or mis-paired element, any early or double rounding and any wrong tail changes bits.

  families    small     iid integers in [-3, 3]
              mantissa  integers in [-127, 127], one in eight from [-255, 255] (the whole 8-bit significand, its
                        last bit included), at K <= 1024, each output row's and each output column's operand
                        row times 2^e, e in [-12, 12]
              onehot    one operand one-hot per output row at a pseudo-random k, the other a position code
                        ((r * 131 + k * 7) mod 251) - 125: every output names the element that was fetched
              slice     `small` with everything outside one 32-deep K slice zeroed
              every family asserts (|A| @ |B|).max() < 2^24 in fp64 on its integer parts
  guards      operands sit inside allocations bordered (rows before / after, gap columns of strided rows) by
              bf16 NaN; outputs are pre-filled with NaN and bordered by a sentinel that must come back intact
  compare     bit patterns; a failure names kernel, case, count, the 256 x 256 tiles, the first triples and,
              for onehot, the element that was actually fetched
  non-linear  GELU / GELU' outputs: |got - ref64| <= 4 |fp32 torch evaluation - ref64| + 1 bf16 ulp(ref64).
              4 is the attention oracle's K with the same reasoning: v_exp_f32 and v_rcp_f32 are ~1 ulp each
              against the ~0.5 ulp of correctly rounded fp32 steps, and the rounding orders differ; the ulp is
              the store's rounding. Column sums: the sum of their summands' allowances + M 2^-24 sum |d|.
              None of this is tuned to make a kernel pass.

Roundings the kernels perform beyond the single one above, read from their sources and part of the expected
values (no tolerance is added for them):
  gemm_ps.hip:330   every epilogue first rounds acc (+ bias) to bf16; DMUL (6) multiplies THAT by c2 (:352) and
                    rounds the product (:354), its column sums add the unrounded fp32 products (:353);
                    DGELU (4) likewise multiplies the bf16-rounded acc by gelu'(c2) (:388-390)
  gemm_ps.hip:368   BIAS_GELU_D (5) / :403 BIAS_GELU (2): gelu, gelu' of the bf16-rounded pre-activation
  gemm.hip:274      DGELU (3): fp32 acc (unrounded) times gelu'(c2), rounded once; :276 the column sums add the
                    ROUNDED bf16 products
  gemm.hip:290      BIAS_GELU (2): gelu of the bf16-rounded pre-activation
"""
from __future__ import annotations

import math
import os
import time
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

EXACT_LIMIT = float(2 ** 24)
TILE = 256
K_NONLINEAR = 4.0
NAN_BITS = 0x7FC0         # bf16 quiet NaN
SENTINEL_BITS = 0x5A5B    # a finite bf16 no test value rounds to
SENTINEL_F32 = -12345.6787109375
GUARD_ROWS = 64
FAMILIES = ("small", "mantissa", "onehot", "slice")
I16 = torch.int16


# ------------------------------------------------------------------------------------ inputs
@dataclass
class Operands:
    """out[i, j] = sum_k A[i, k] B[j, k] (+ bias[j]); float64 CPU tensors holding bf16-exact values."""
    A: torch.Tensor
    B: torch.Tensor
    bias: torch.Tensor
    family: str
    hot: torch.Tensor | None = None   # onehot: the k each row of A selects
    info: dict = field(default_factory=dict)  # mantissa: "cb", the power of two of each row of B (output column)

    @property
    def exact(self):
        """A B^T in float64, computed once."""
        if "exact" not in self.info:
            self.info["exact"] = self.A @ self.B.t()
        return self.info["exact"]


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64)


def _ints8(g, shape):
    """mantissa: integers in [-127, 127], one entry in eight redrawn from [-255, 255]. 127 has only 7 significant
    bits, so with [-127, 127] alone the last bit of the bf16 significand is never set and an operand that loses it
    goes unseen; the redrawn odd values set it. Exactness stays a checked condition (assert_exact)."""
    v, wide = _ints(g, -127, 127, shape), _ints(g, -255, 255, shape)
    return torch.where(torch.rand(shape, generator=g) < 0.125, wide, v)


def assert_exact(A, B, what=""):
    """The checked condition for exactness: on the integer parts, sum |a| |b| < 2^24 (so every partial sum in
    any order is an integer below 2^24 and fp32 holds it)."""
    bound = float((A.abs() @ B.abs().t()).max())
    assert bound < EXACT_LIMIT, f"{what}: sum |a||b| = {bound} is not below 2^24: fp32 partial sums may round"
    return bound


def position_code(r, k):
    return ((r * 131 + k * 7) % 251) - 125


def make_nt(family, R, C, K, seed=0, live=None):
    """Operands of one family for out [R, C], depth K. live: the 32-deep K slice kept by `slice`."""
    g = _gen(seed * 7919 + R * 31 + C * 17 + K)
    hot = None
    if family in ("small", "slice"):
        A, B, bias = _ints(g, -3, 3, (R, K)), _ints(g, -3, 3, (C, K)), _ints(g, -3, 3, (C,))
        if family == "slice":
            assert live is not None and 0 <= live < K // 32, (live, K)
            keep = torch.zeros(K, dtype=torch.bool)
            keep[live * 32:(live + 1) * 32] = True
            zero = torch.zeros((), dtype=torch.float64)  # (not a product with 0: that would leave -0.0 entries)
            A, B = torch.where(keep, A, zero), torch.where(keep, B, zero)
        assert_exact(A, B, family)
    elif family == "mantissa":
        assert K <= 1024, "mantissa: [-127, 127] stays exact up to K = 1024"
        A, B, bias = _ints8(g, (R, K)), _ints8(g, (C, K)), _ints(g, -127, 127, (C,))
        assert_exact(A, B, family)
        ra = torch.exp2(_ints(g, -12, 12, (R,)))
        cb = torch.exp2(_ints(g, -12, 12, (C,)))
        A, B, bias = A * ra[:, None], B * cb[:, None], bias * cb
    elif family == "onehot":
        hot = (torch.arange(R, dtype=torch.int64) * 2654435761 + seed * 97 + 13) % K
        A = torch.zeros(R, K, dtype=torch.float64)
        A[torch.arange(R), hot] = 1.0
        B = position_code(torch.arange(C)[:, None], torch.arange(K)[None, :]).to(torch.float64)
        bias = torch.zeros(C, dtype=torch.float64)
        assert_exact(A, B, family)
    else:
        raise ValueError(family)
    for t in (A, B, bias):  # bf16 holds every value
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    return Operands(A, B, bias, family, hot, {"live": live, "cb": cb if family == "mantissa" else None})


def int_base(shape, family, seed=0, colscale=None):
    """An integer-valued accumulate base / c2 (mantissa: times the column's power of two)."""
    g = _gen(seed * 104729 + 5)
    if family == "mantissa":
        b = _ints(g, -127, 127, shape)
        return b * colscale if colscale is not None else b
    return _ints(g, -3, 3, shape)


def live_slices(nslices, splits=1):
    """The live slices the `slice` family is run over: the first, slices 3 and 4 (the 4-slot ring's wrap), the
    last, and the first and last slice of every split (splits over 64-deep blocks as gemm_wg.hip:90 does)."""
    s = {0, 3, 4, nslices - 1}
    nb = nslices // 2
    for i in range(splits):
        s.add(2 * (i * nb // splits))
        s.add(2 * ((i + 1) * nb // splits) - 1)
    return sorted(x for x in s if 0 <= x < nslices)


def gelu_operands(R, C, K, seed=0):
    """Integer operands and bias whose pre-activation A B^T + bias stays within [-8, 8] and covers both tails
    and the region around 0: three +-1 entries per row of A, B in [-2, 2], bias in [-2, 2]."""
    g = _gen(seed * 613 + R + C + K)
    A = torch.zeros(R, K, dtype=torch.float64)
    for _ in range(3):
        k = torch.randint(0, K, (R,), generator=g)
        A[torch.arange(R), k] = _ints(g, 0, 1, (R,)) * 2 - 1
    B, bias = _ints(g, -2, 2, (C, K)), _ints(g, -2, 2, (C,))
    assert_exact(A, B, "gelu")
    pre = A @ B.t() + bias
    assert float(pre.abs().max()) <= 8 and float(pre.min()) <= -6 and float(pre.max()) >= 6 and bool((pre == 0).any())
    return Operands(A, B, bias, "gelu")


# ------------------------------------------------------------------------------------ expected values
def to_bf16(x64):
    """The kernels' single rounding: the exact value through one fp32 operation, then the bf16 store. + 0.0
    makes an exact zero +0 as the accumulators have it."""
    return (x64 + 0.0).to(torch.float32).to(torch.bfloat16)


def bf(x64):
    """to_bf16 as float64 values (a rounding inside an expected-value model)."""
    return to_bf16(x64).double()


def expected_nt(op, bias=False, base=None):
    exact = op.exact
    if bias:
        exact = exact + op.bias
    if base is not None:
        exact = exact + base
    return to_bf16(exact)


# NHWC convolution references, float64 on the CPU. w: [Cout, 3, 3, Cin]
def conv_ref(x, w, stride):
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=1).permute(0, 2, 3, 1)


def conv_wgrad_ref(x, dy, stride):
    """[Cout, 9 Cin] in the [Cout][ky][kx][Cin] layout."""
    cout, cin = dy.shape[3], x.shape[3]
    r = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (cout, cin, 3, 3), dy.permute(0, 3, 1, 2), stride=stride,
                                    padding=1)
    return r.permute(0, 2, 3, 1).reshape(cout, 9 * cin)


def conv_dgrad_ref(dy, w):
    """Stride-1 input gradient of conv(x, w), w [Cout, 3, 3, Cin], dy NHWC [.., Cout] -> NHWC [.., Cin]."""
    n, h, wd, _ = dy.shape
    wn = w.permute(0, 3, 1, 2).contiguous()
    x = torch.zeros(n, wn.shape[1], h, wd, dtype=dy.dtype)
    return torch.ops.aten.convolution_backward(dy.permute(0, 3, 1, 2).contiguous(), x, wn, None, [1, 1], [1, 1], [1, 1],
                                               False, [0, 0], 1, [True, False, False])[0].permute(0, 2, 3, 1)


def conv_code(imgs, H, W, C):
    """onehot for the conv modes: x holds a code of (img, y, x, c), so a wrong tap, pixel or channel is read off
    the value."""
    i, y, xx, c = torch.meshgrid(torch.arange(imgs), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    return (((i * 131 + y * 37 + xx * 7 + c * 3) % 251) - 125).to(torch.float64)


def conv_decode(value, imgs, H, W, C, limit=4):
    code = conv_code(imgs, H, W, C)
    hits = (code == float(value)).nonzero()[:limit]
    return [tuple(int(v) for v in h) for h in hits]


def make_conv(family, imgs, H, W, Cin, Cout, stride, seed=0, wgrad=False):
    """x [imgs, H, W, Cin] and the other operand -- w [Cout, 3, 3, Cin] (forward) or dy [imgs, Ho, Wo, Cout]
    (wgrad) -- plus a bias [Cout], float64. mantissa scales the output channel only (x feeds every output)."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = _gen(seed * 7919 + imgs * 131 + H * 17 + W * 5 + Cin + Cout + stride)
    oshape = (imgs, Ho, Wo, Cout) if wgrad else (Cout, 3, 3, Cin)
    if family == "small":
        x, o, bias = _ints(g, -3, 3, (imgs, H, W, Cin)), _ints(g, -3, 3, oshape), _ints(g, -3, 3, (Cout,))
    elif family == "mantissa":
        depth = imgs * Ho * Wo if wgrad else 9 * Cin
        assert depth <= 1024, "mantissa: accumulated depth <= 1024"
        x, o, bias = _ints8(g, (imgs, H, W, Cin)), _ints8(g, oshape), _ints(g, -127, 127, (Cout,))
        sc = torch.exp2(_ints(g, -12, 12, (Cout,)))
        o = o * (sc if wgrad else sc[:, None, None, None])
        bias = bias * sc
    elif family == "onehot":
        x = conv_code(imgs, H, W, Cin)
        o = torch.zeros(oshape, dtype=torch.float64)
        co = torch.arange(Cout)
        if wgrad:  # each output channel picks one token
            t = (co * 2654435761 + seed * 97 + 13) % (imgs * Ho * Wo)
            o.view(-1, Cout)[t, co] = 1.0
        else:      # each output channel picks one (tap, channel)
            kk = (co * 2654435761 + seed * 97 + 13) % (9 * Cin)
            o.view(Cout, -1)[co, kk] = 1.0
        bias = torch.zeros(Cout, dtype=torch.float64)
    else:
        raise ValueError(family)
    ax, ao = x.abs(), o.abs()
    if family == "mantissa":  # the integer parts
        ao = ao / (sc if wgrad else sc[:, None, None, None])
    bound = float((conv_wgrad_ref(ax, ao, stride) if wgrad else conv_ref(ax, ao, stride)).max())
    assert bound < EXACT_LIMIT, f"conv {family}: sum |a||b| = {bound} is not below 2^24"
    return x, o, bias


# ------------------------------------------------------------------------------------ guard bands
class Guarded:
    """A bf16 [R, C] matrix (or a contiguous N-D tensor: rows = all but the last dim) placed as a view inside a
    larger allocation: GUARD_ROWS rows of `border` bits before and after, and the gap columns C..ld of every
    row. Operands: border = NaN. Outputs: border = the sentinel and the view pre-filled with NaN (or a base)."""

    def __init__(self, shape, device, ld=None, border=NAN_BITS, value=None):
        self.shape = tuple(shape)
        C = self.shape[-1]
        R = 1
        for s in self.shape[:-1]:
            R *= s
        self.R, self.C, self.ld = R, C, ld or C
        assert self.ld >= C and self.ld % 8 == 0 and (len(self.shape) == 2 or self.ld == C)
        self.border = border
        self.whole = torch.full(((R + 2 * GUARD_ROWS) * self.ld,), border, dtype=I16).to(device)
        rows = self.whole.view(torch.bfloat16)[GUARD_ROWS * self.ld:(GUARD_ROWS + R) * self.ld].view(R, self.ld)
        self.view = rows[:, :C] if len(self.shape) == 2 else rows.view(self.shape)
        if value is None:
            self.view.view(I16).fill_(NAN_BITS)
        else:
            self.view.copy_(value.to(torch.bfloat16).reshape(self.view.shape))

    def border_intact(self):
        """True when every element outside the view still holds the border bits."""
        w = self.whole.cpu().view(-1, self.ld)
        inner = torch.zeros(w.shape, dtype=torch.bool)
        inner[GUARD_ROWS:GUARD_ROWS + self.R, :self.C] = True
        return bool((w[~inner] == self.border).all())

    def result(self):
        return self.view.detach().cpu().reshape(self.R, self.C).contiguous()


def operand(value64, device, ld=None):
    """value64 (float64, bf16-exact) as a NaN-bordered device operand view."""
    return Guarded(value64.shape, device, ld=ld, border=NAN_BITS, value=value64).view


def output(shape, device, ld=None, base=None):
    """A sentinel-bordered output, pre-filled with NaN (or holding `base` for an accumulate)."""
    return Guarded(shape, device, ld=ld, border=SENTINEL_BITS, value=base)


class GuardedF32:
    """fp32 [N] (column sums) between two sentinel bands, zeroed."""

    def __init__(self, n, device):
        self.n = n
        self.whole = torch.full((n + 2 * GUARD_ROWS,), SENTINEL_F32, dtype=torch.float32, device=device)
        self.view = self.whole[GUARD_ROWS:GUARD_ROWS + n]
        self.view.zero_()

    def border_intact(self):
        w = self.whole.cpu()
        return bool((w[:GUARD_ROWS] == SENTINEL_F32).all() and (w[GUARD_ROWS + self.n:] == SENTINEL_F32).all())

    def result(self):
        return self.view.detach().cpu().clone()


# ------------------------------------------------------------------------------------ comparison
def mismatch_report(got, want, kernel, case, decode=None, limit=5):
    """None when got and want (2-D, same dtype) are bit-identical, else the failure message."""
    assert got.shape == want.shape and got.dtype == want.dtype and got.dim() == 2, (got.shape, want.shape)
    it = I16 if got.dtype == torch.bfloat16 else torch.int32
    gb, wb = got.contiguous().view(it), want.contiguous().view(it)
    if torch.equal(gb, wb):
        return None
    bad = (gb != wb).nonzero()
    tiles = sorted({(int(r) // TILE, int(c) // TILE) for r, c in bad[:100000]})
    lines = [f"{kernel} {case}: {bad.shape[0]} of {got.numel()} elements differ from the exact result; "
             f"256 x 256 tiles (row tile, column tile): {tiles[:24]}{' ...' if len(tiles) > 24 else ''}"]
    for r, c in bad[:limit]:
        r, c = int(r), int(c)
        line = f"  [{r}, {c}] got {float(got[r, c])!r} want {float(want[r, c])!r}"
        if decode is not None:
            line += f"; fetched {decode(r, c, float(got[r, c]))}"
        lines.append(line)
    return "\n".join(lines)


def assert_bits(got, want, kernel, case, decode=None):
    """Bit-pattern equality of a kernel output with the expected values; records the case."""
    msg = mismatch_report(got, want, kernel, case, decode)
    it = I16 if got.dtype == torch.bfloat16 else torch.int32
    record(kernel, case, got.numel(), int((got.contiguous().view(it) != want.contiguous().view(it)).sum()))
    assert msg is None, msg


def nt_decoder(op):
    """onehot: which (row of B, k) holds the value that came out at [r, c], and what should have been read."""
    K = op.B.shape[1]

    def decode(r, c, v):
        ks = [k for k in range(K) if float(op.B[c, k]) == v][:4]
        return f"B[{c}, k in {ks}] (row {r} selects k = {int(op.hot[r])})"
    return decode


# ------------------------------------------------------------------------------------ non-linear epilogues
_S2PI = math.sqrt(2.0 / math.pi)


def gelu_tanh(x):
    """tanh-GELU in the dtype of x (float64: the reference; float32: the plain torch evaluation whose error
    against float64 sizes the allowance), written x sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3): the same
    function as 0.5 x (1 + tanh u), whose literal form cancels to -0.0 in float64 below x = -5.6 (at x = -8
    the value is -3.1e-21, and the kernels deliver it)."""
    return x * torch.sigmoid(2.0 * _S2PI * (x + 0.044715 * x * x * x))


def gelu_tanh_grad(x):
    """d/dx [x sigmoid(2u)] = s + x s (1 - s) (2u)', with 1 - s taken as sigmoid(-2u) (no cancellation)."""
    z = 2.0 * _S2PI * (x + 0.044715 * x * x * x)
    s = torch.sigmoid(z)
    return s + x * s * torch.sigmoid(-z) * (2.0 * _S2PI * (1.0 + 3.0 * 0.044715 * x * x))


def ulp_bf16(x64):
    """One unit in the last place of bf16 at |x| (0 at 0)."""
    _, e = torch.frexp(x64.abs())
    return torch.where(x64 == 0, torch.zeros_like(x64), torch.exp2((e - 8).double()))


def allowance(ref64, model32, final_rounding=True):
    a = K_NONLINEAR * (model32.double() - ref64).abs()
    return a + ulp_bf16(ref64) if final_rounding else a


def assert_within(got, ref64, allow, kernel, case):
    """|got - ref64| <= allow elementwise (2-D or 1-D); returns and records the worst error / allowance."""
    g = got.double()
    assert g.shape == ref64.shape, (g.shape, ref64.shape)
    err = (g - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / allow)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    exact = to_bf16(ref64).double() if got.dtype == torch.bfloat16 else ref64.float().double()
    record(kernel, case, got.numel(), int((g != exact).sum()), worst)
    if not worst <= 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        n = int((ratio > 1.0).sum())
        raise AssertionError(f"{kernel} {case}: {n} elements outside the allowance; worst at {idx}: got "
                             f"{float(g.flatten()[i])!r}, float64 reference {float(ref64.flatten()[i])!r}, error "
                             f"{float(err.flatten()[i]):.4g} is {worst:.3g}x the allowance {float(allow.flatten()[i]):.4g}")
    return worst


# ------------------------------------------------------------------------------------ record
_CASES: dict = {}
_T0 = [None]


def record(kernel, case, elems, not_equal, ratio=None):
    """Per kernel: cases run, elements compared, elements not bit-equal to the rounded float64 value and, for
    the non-linear outputs, the worst error / allowance. With GEMM_ORACLE_REPORT=<path> in the environment the
    table is rewritten there after every update (profiles/gemm_oracle.txt is one GPU run of
    tests/test_gemm_oracle_gpu.py written this way)."""
    if _T0[0] is None:
        _T0[0] = time.time()
    k = _CASES.setdefault(kernel, {"cases": set(), "elems": 0, "ne": 0, "nl_elems": 0, "nl_ne": 0, "ratio": 0.0})
    k["cases"].add(case)
    if ratio is None:
        k["elems"] += elems
        k["ne"] += not_equal
    else:
        k["nl_elems"] += elems
        k["nl_ne"] += not_equal
        k["ratio"] = max(k["ratio"], ratio)
    path = os.environ.get("GEMM_ORACLE_REPORT")
    if not path:
        return
    lines = ["# tests/test_gemm_oracle_gpu.py: exact (integer) families must be bit-equal to the rounded float64 "
             "result (share 0);",
             f"# non-linear outputs: worst error / allowance (bound 1; allowance = {K_NONLINEAR:g} x the fp32 "
             "model's own error + 1 bf16 ulp)",
             f"{'kernel':<18} {'cases':>5} {'exact elems':>12} {'not bit-equal':>13} {'non-lin elems':>13} "
             f"{'not bit-equal':>13} {'worst ratio':>11}"]
    for name, k in sorted(_CASES.items()):
        s1 = f"{k['ne'] / k['elems']:.2e}" if k["elems"] else "-"
        s2 = f"{k['nl_ne'] / k['nl_elems']:.2e}" if k["nl_elems"] else "-"
        r = f"{k['ratio']:.3f}" if k["nl_elems"] else "-"
        lines.append(f"{name:<18} {len(k['cases']):>5} {k['elems']:>12} {s1:>13} {k['nl_elems']:>13} {s2:>13} {r:>11}")
    lines.append(f"# wall time since the first comparison: {time.time() - _T0[0]:.1f} s")
    for name, k in sorted(_CASES.items()):
        lines += ["", f"# {name}: the cases run"] + [f"  {c}" for c in sorted(k["cases"])]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
