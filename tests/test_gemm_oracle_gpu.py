"""The hand-written GEMM and implicit-GEMM convolution kernels (gemm_wg, gemm_wg_conv3x3, gemm_f, gemm_f_conv3x3,
gemm_ps, gemm_nt) against the exact-arithmetic oracle of tests/_gemm_oracle.py: integer-valued bf16 operands make
the float64 result, rounded once, the ONLY correct bit pattern, so the exact families allow zero differing elements;
the GELU epilogues get 4 x the fp32 model's own error plus one bf16 ulp. Every operand sits in a NaN-bordered
allocation, every output is pre-filled with NaN inside a sentinel border. The shapes are the smallest that reach each
mechanism (the shortest pipelines, ragged splits and panels, images smaller than a slice, one workgroup walking every
tile). Every case first asserts the kernel's own *_supported call, so a refusal cannot turn into a silent skip."""
import functools

import pytest
import torch

from tests import _gemm_oracle as go

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C(gpu):
    from distributedvolunteercomputing_amd.ops import native

    return native()


@functools.lru_cache(maxsize=64)
def _ops(family, R, Cc, K, live=None, seed=0):
    return go.make_nt(family, R, Cc, K, seed, live)


@functools.lru_cache(maxsize=16)
def _gelu_ops(R, Cc, K):
    return go.gelu_operands(R, Cc, K)


def _families(K):
    return ("small", "mantissa") if K <= 1024 else ("small",)


def _decode(op):
    return go.nt_decoder(op) if op.family == "onehot" else None


def _tag(op):
    return op.family + (f"[{op.info['live']}]" if op.family == "slice" else "")


# ------------------------------------------------------------------------------------ gemm_wg
# (K tokens, M, N, splits): out[M, N] = a[K, M]^T b[K, N]
WG_SHAPES = [(192, 256, 256, 1),    # nk = 6, the shortest pipeline
             (256, 256, 256, 1),    # nk = 8
             (384, 256, 256, 2),    # every split at nk = 6
             (448, 256, 256, 2),    # ragged splits of 3 and 4 blocks
             (1088, 256, 512, 5),   # ragged splits
             (192, 128, 256, 1),    # a lone half panel
             (384, 384, 512, 2),    # 1.5 panels
             (1536, 512, 512, 3),   # 12 workgroups: the XCD order with more than one tile and split
             (4096, 768, 768, 0)]   # default splits


def _wg_run(C, gpu, op, splits, loaders, accumulate, lda=None, ldb=None, note="", repeats=1):
    M, N, K = op.A.shape[0], op.B.shape[0], op.A.shape[1]
    assert C.gemm_wg_supported(M, N, K, splits)
    a = go.operand(op.A.t().contiguous(), gpu, ld=lda)
    b = go.operand(op.B.t().contiguous(), gpu, ld=ldb)
    base = go.int_base((M, N), op.family, seed=K, colscale=op.info["cb"]) if accumulate else None
    want = go.expected_nt(op, base=base)
    for rep in range(repeats):
        out = go.output((M, N), gpu, base=base)
        C.gemm_wg(a, b, out.view, accumulate, splits, loaders)
        case = f"K{K} M{M} N{N} s{splits} l{loaders} acc{int(accumulate)} {_tag(op)}{note}"
        go.assert_bits(out.result(), want, "gemm_wg", case, _decode(op))
        assert out.border_intact(), f"gemm_wg {case}: wrote outside its output"


@pytest.mark.parametrize("K,M,N,splits", WG_SHAPES)
def test_gemm_wg_exact(C, gpu, K, M, N, splits):
    for fam in _families(K):
        op = _ops(fam, M, N, K)
        for loaders in (8, 4):
            for accumulate in (False, True):
                _wg_run(C, gpu, op, splits, loaders, accumulate)


@pytest.mark.parametrize("K,M,N,splits", [(448, 256, 256, 2), (1088, 256, 512, 5)])
def test_gemm_wg_onehot_and_slices(C, gpu, K, M, N, splits):
    for loaders in (8, 4):
        _wg_run(C, gpu, _ops("onehot", M, N, K), splits, loaders, False)
        for live in go.live_slices(K // 32, splits):
            _wg_run(C, gpu, _ops("slice", M, N, K, live), splits, loaders, False)


def test_gemm_wg_strided_rows(C, gpu):
    """lda > M and ldb > N separately; the gap columns are NaN."""
    K, M, N, splits = 384, 384, 512, 2
    for fam in ("small", "mantissa"):
        op = _ops(fam, M, N, K)
        for loaders in (8, 4):
            _wg_run(C, gpu, op, splits, loaders, False, lda=M + 64, note=" lda")
            _wg_run(C, gpu, op, splits, loaders, True, ldb=N + 128, note=" ldb")


def test_gemm_wg_three_runs_equal_the_truth(C, gpu):
    for loaders in (8, 4):
        _wg_run(C, gpu, _ops("small", 512, 512, 1536), 3, loaders, False, note=" x3", repeats=3)


# ------------------------------------------------------------------------------------ gemm_wg_conv3x3
# (imgs, H, W, Cin, Cout, stride, explicit splits)
WGC_SHAPES = [(12, 4, 4, 128, 128, 1, 1),    # an image of 16 tokens < one 32-token slice: the carry wraps rows and images
              (3, 8, 8, 128, 256, 1, 1),
              (1, 8, 40, 256, 128, 1, 1),    # Wo > 32
              (3, 15, 15, 128, 128, 2, 1),   # odd H at stride 2
              (3, 16, 16, 256, 256, 2, 1),   # even H at stride 2: only the top and left padding is touched
              (6, 8, 8, 128, 128, 1, 2)]     # a split boundary in mid-image


@functools.lru_cache(maxsize=32)
def _wgc_ops(family, imgs, H, W, cin, cout, stride, live=None):
    x, dy, _ = go.make_conv("small" if family == "slice" else family, imgs, H, W, cin, cout, stride, wgrad=True)
    if family == "slice":  # only one 32-token slice of dy alive
        keep = torch.zeros(dy.shape[0] * dy.shape[1] * dy.shape[2], dtype=torch.bool)
        keep[live * 32:(live + 1) * 32] = True
        dy = torch.where(keep.view(dy.shape[:3])[..., None], dy, torch.zeros((), dtype=torch.float64))
    return x, dy, go.conv_wgrad_ref(x, dy, stride)


def _wgc_run(C, gpu, family, shape, splits, accumulate, live=None, repeats=1):
    imgs, H, W, cin, cout, stride = shape
    assert C.gemm_wg_conv3x3_supported(cout, cin, imgs, H, W, stride)
    x, dy, exact = _wgc_ops(family, imgs, H, W, cin, cout, stride, live)
    # (any bf16 base keeps the model exact: base + sum is ONE fp32 addition of exact values, then the bf16 store)
    base = go.int_base(exact.shape, family if family == "mantissa" else "small", seed=H) if accumulate else None
    want = go.to_bf16(exact + base if accumulate else exact)
    xg, dyg = go.operand(x, gpu), go.operand(dy, gpu)
    case = f"{shape} s{splits} acc{int(accumulate)} {family}{'' if live is None else [live]}"

    def decode(r, c, v):
        return f"x[img, y, x, c] in {go.conv_decode(v, imgs, H, W, cin)} for out[co {r}, tap {c // cin}, c {c % cin}]"

    for _ in range(repeats):
        out = go.output(exact.shape, gpu, base=base)
        C.gemm_wg_conv3x3(dyg, xg, out.view, accumulate, stride, splits)
        go.assert_bits(out.result(), want, "gemm_wg_conv3x3", case, decode if family == "onehot" else None)
        assert out.border_intact(), f"gemm_wg_conv3x3 {case}: wrote outside its output"


@pytest.mark.parametrize("imgs,H,W,cin,cout,stride,splits", WGC_SHAPES)
def test_gemm_wg_conv3x3_exact(C, gpu, imgs, H, W, cin, cout, stride, splits):
    shape = (imgs, H, W, cin, cout, stride)
    for fam in ("small", "mantissa"):  # every shape accumulates <= 384 tokens
        for s in (0, splits):
            for accumulate in (False, True):
                _wgc_run(C, gpu, fam, shape, s, accumulate)


@pytest.mark.parametrize("imgs,H,W,cin,cout,stride,splits", [WGC_SHAPES[0], WGC_SHAPES[3], WGC_SHAPES[5]])
def test_gemm_wg_conv3x3_onehot_and_slices(C, gpu, imgs, H, W, cin, cout, stride, splits):
    shape = (imgs, H, W, cin, cout, stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    _wgc_run(C, gpu, "onehot", shape, splits, False)
    for live in go.live_slices(imgs * Ho * Wo // 32, splits):
        _wgc_run(C, gpu, "slice", shape, splits, False, live=live)


def test_gemm_wg_conv3x3_three_runs_equal_the_truth(C, gpu):
    _wgc_run(C, gpu, "small", WGC_SHAPES[5][:6], 2, False, repeats=3)


# ------------------------------------------------------------------------------------ gemm_f
F_SHAPES = [(1, 64, 192), (255, 128, 192), (257, 128, 256), (300, 384, 256), (256, 256, 192), (513, 640, 320),
            (300, 64, 256),      # the 256 x 64 tile with a ragged second row panel
            (1300, 384, 192)]    # 6 row panels: grouped_tile's last group of 2 (GROUP_M = 4), 12 workgroups


def _f_run(C, gpu, op, waves, bias, splits=-2, lda=None, ldb=None, ldc=None, note="", repeats=1):
    """splits = -2: the plain call (one split)."""
    M, N, K = op.A.shape[0], op.B.shape[0], op.A.shape[1]
    assert C.gemm_f_supported(M, N, K)
    a, b = go.operand(op.A, gpu, ld=lda), go.operand(op.B, gpu, ld=ldb)
    bg = go.operand(op.bias[None, :], gpu)[0] if bias else None
    want = go.expected_nt(op, bias=bias)
    case = f"M{M} N{N} K{K} w{waves} b{int(bias)} s{splits} {_tag(op)}{note}"
    for _ in range(repeats):
        out = go.output((M, N), gpu, ld=ldc)
        if splits == -2:
            C.gemm_f(a, b, out.view, bg, waves)
        else:
            C.gemm_f(a, b, out.view, bg, waves, splits)
        go.assert_bits(out.result(), want, "gemm_f", case, _decode(op))
        assert out.border_intact(), f"gemm_f {case}: wrote outside its output"


def _waves(N):
    return (4, 8) if N >= 256 else (8,)


@pytest.mark.parametrize("M,N,K", F_SHAPES)
def test_gemm_f_exact(C, gpu, M, N, K):
    for fam in _families(K):
        op = _ops(fam, M, N, K)
        for waves in _waves(N):
            for bias in (False, True):
                _f_run(C, gpu, op, waves, bias)


@pytest.mark.parametrize("M,N,K,splits", [(512, 256, 384, 2), (300, 384, 768, 4), (300, 384, 768, -1)])
def test_gemm_f_split_k_exact(C, gpu, M, N, K, splits):
    if splits < 0:
        assert C.gemm_f_splits(M, N, K) > 1
    for fam in _families(K):
        op = _ops(fam, M, N, K)
        for waves in _waves(N):
            for bias in (False, True):
                _f_run(C, gpu, op, waves, bias, splits=splits, ldc=N + 64, note=" ldc")
    ns = splits if splits > 0 else C.gemm_f_splits(M, N, K)
    for live in go.live_slices(K // 32, ns):
        _f_run(C, gpu, _ops("slice", M, N, K, live), 8, True, splits=splits, ldc=N + 64, note=" ldc")


@pytest.mark.parametrize("M,N,K", [(300, 384, 256), (513, 640, 320)])
def test_gemm_f_onehot_slices_and_strides(C, gpu, M, N, K):
    for waves in (4, 8):
        _f_run(C, gpu, _ops("onehot", M, N, K), waves, False)
        for live in go.live_slices(K // 32):
            _f_run(C, gpu, _ops("slice", M, N, K, live), waves, True)
        op = _ops("small", M, N, K)
        _f_run(C, gpu, op, waves, True, lda=K + 64, note=" lda")
        _f_run(C, gpu, op, waves, True, ldb=K + 128, note=" ldb")
        _f_run(C, gpu, op, waves, True, lda=K + 8, ldb=K + 8, ldc=N + 8, note=" lda ldb ldc")


def test_gemm_f_three_runs_equal_the_truth(C, gpu):
    for waves in (4, 8):
        _f_run(C, gpu, _ops("small", 513, 640, 320), waves, True, note=" x3", repeats=3)
    _f_run(C, gpu, _ops("small", 300, 384, 768), 8, True, splits=4, ldc=448, note=" x3", repeats=3)


# ------------------------------------------------------------------------------------ gemm_f_conv3x3
FC_SHAPES = [(1, 1, 1, 64, 64, 1),      # every tap but the centre is padding
             (2, 1, 9, 64, 128, 1), (2, 9, 1, 128, 64, 1), (3, 5, 6, 64, 384, 2), (2, 7, 7, 64, 128, 2),
             (3, 8, 8, 128, 256, 2),
             (4, 7, 7, 512, 512, 1)]    # takes the automatic split-K
FC_MODES = ("plain", "flip", "tapmajor", "tapmajor_flip")


@functools.lru_cache(maxsize=16)
def _fc_ops(family, imgs, H, W, cin, cout, stride):
    x, w, bias = go.make_conv(family, imgs, H, W, cin, cout, stride)
    plain = go.conv_ref(x, w, stride)
    flipped = go.conv_ref(x, w.flip(1, 2), stride)  # gemm_f.hip:147: weight tap (ky, kx) meets pixel tap (2 - ky, 2 - kx)
    if stride == 1:
        # ... which is the stride-1 input gradient of the convolution whose weight is w with its channel axes swapped
        # ([Cout_conv = Cin_call][ky][kx][Cin_conv = Cout_call]): the float64 convolution_backward agrees exactly
        assert torch.equal(go.conv_dgrad_ref(x, w.permute(3, 1, 2, 0).contiguous()), flipped)
    return x, w, bias, plain, flipped


def _fc_run(C, gpu, family, shape, mode, waves, bias, repeats=1):
    imgs, H, W, cin, cout, stride = shape
    assert C.gemm_f_conv3x3_supported(imgs, H, W, cin, cout, stride)
    x, w, bvec, plain, flipped = _fc_ops(family, *shape)
    exact = flipped if mode.endswith("flip") else plain
    if bias:
        exact = exact + bvec
    want = go.to_bf16(exact).reshape(-1, cout)
    wk = w.reshape(cout, 9, cin).permute(1, 0, 2).contiguous() if mode.startswith("tapmajor") else w
    xg, wg = go.operand(x, gpu), go.operand(wk, gpu)
    bg = go.operand(bvec[None, :], gpu)[0] if bias else None
    case = f"{shape} {mode} w{waves} b{int(bias)} {family}"

    def decode(r, c, v):
        return f"x[img, y, x, c] in {go.conv_decode(v, imgs, H, W, cin)} for pixel {r}, output channel {c}"

    for _ in range(repeats):
        out = go.output(exact.shape, gpu)
        C.gemm_f_conv3x3(xg, wg, out.view, stride, bg, waves, -1, mode.endswith("flip"))
        go.assert_bits(out.result(), want, "gemm_f_conv3x3", case, decode if family == "onehot" else None)
        assert out.border_intact(), f"gemm_f_conv3x3 {case}: wrote outside its output"


@pytest.mark.parametrize("imgs,H,W,cin,cout,stride", FC_SHAPES)
def test_gemm_f_conv3x3_exact(C, gpu, imgs, H, W, cin, cout, stride):
    shape = (imgs, H, W, cin, cout, stride)
    if cin == 512:
        assert C.gemm_f_splits(imgs * H * W, cout, 9 * cin) > 1
    for fam in _families(9 * cin):
        for mode in FC_MODES:
            for waves in _waves(cout):
                for bias in (False, True):
                    _fc_run(C, gpu, fam, shape, mode, waves, bias)


@pytest.mark.parametrize("imgs,H,W,cin,cout,stride", [FC_SHAPES[3], FC_SHAPES[4]])
def test_gemm_f_conv3x3_onehot(C, gpu, imgs, H, W, cin, cout, stride):
    for mode in FC_MODES:
        for waves in _waves(cout):
            _fc_run(C, gpu, "onehot", (imgs, H, W, cin, cout, stride), mode, waves, False)


def test_gemm_f_conv3x3_three_runs_equal_the_truth(C, gpu):
    _fc_run(C, gpu, "small", FC_SHAPES[5], "plain", 8, True, repeats=3)
    _fc_run(C, gpu, "small", FC_SHAPES[6], "tapmajor_flip", 8, False, repeats=3)


# ------------------------------------------------------------------------------------ gemm_ps / gemm_nt
# (M, N, K, grid_cap)
PS_SHAPES = [(256, 256, 256, 0),     # nk = 8, the shortest K
             (256, 256, 384, 0),
             (1024, 512, 256, 1),    # one workgroup walks all 8 tiles through one ring
             (1280, 512, 384, 3),    # tiles not divisible by the grid
             (768, 768, 512, 2)]


def _launch(C, kernel, a, b, c, c2, bias, cs, epi, cap):
    if kernel == "gemm_ps":
        C.gemm_ps(a, b, c, c2, bias, cs, epi, cap)
    else:
        C.gemm_nt(a, b, c, c2, bias, cs, epi)


def _supported(C, kernel, M, N, K, epi):
    return C.gemm_ps_supported(M, N, K, epi) if kernel == "gemm_ps" else C.gemm_nt_supported_epi(M, N, K, epi)


def _epi_exact(C, gpu, kernel, op, epi, cap=0, lda=None, ldc=None, note="", repeats=1):
    """Store / bias (/ bias + ReLU, gemm_nt's 4) and gemm_ps's DMUL (6) epilogues: bit-exact."""
    M, N, K = op.A.shape[0], op.B.shape[0], op.A.shape[1]
    assert _supported(C, kernel, M, N, K, epi)
    a, b = go.operand(op.A, gpu, ld=lda), go.operand(op.B, gpu)
    case = f"M{M} N{N} K{K} cap{cap} epi{epi} {_tag(op)}{note}"
    bg = c2v = None
    if epi == 6:
        c2v = go.int_base((M, N), "small", seed=M + K)
        g = go.bf(op.exact)                  # gemm_ps.hip:330 acc -> bf16 before the multiply
        d = g * c2v                          # :352 fp32 product of two bf16 values: exact
        assert float(d.abs().sum(0).max()) < go.EXACT_LIMIT  # integer column sums: exact in any order
        # :354 / :353 (no + 0.0 here: 0 times a negative c2 is -0.0 in the kernel's fp32 product and in d alike)
        want, want_cs = d.to(torch.float32).to(torch.bfloat16), (d.sum(0) + 0.0).to(torch.float32)
    else:
        bg = go.operand(op.bias[None, :], gpu)[0] if epi in (1, 4) else None
        exact = op.exact + op.bias if epi in (1, 4) else op.exact
        want = go.to_bf16(exact.clamp_min(0.0) if epi == 4 else exact)  # gemm.hip:269
    for _ in range(repeats):
        out = go.output((M, N), gpu, ld=ldc)
        c2 = go.output((M, N), gpu, ld=ldc, base=c2v) if epi == 6 else None
        cs = go.GuardedF32(N, gpu) if epi == 6 else None
        _launch(C, kernel, a, b, out.view, c2.view if c2 else None, bg, cs.view if cs else None, epi, cap)
        go.assert_bits(out.result(), want, kernel, case, _decode(op))
        assert out.border_intact(), f"{kernel} {case}: wrote outside its output"
        if epi == 6:
            go.assert_bits(cs.result()[None, :], want_cs[None, :], kernel, case + " colsum")
            assert cs.border_intact() and c2.border_intact()
            assert torch.equal(c2.result().view(go.I16), go.to_bf16(c2v).view(go.I16)), f"{kernel} {case}: c2 changed"


def _epi_gelu(C, gpu, kernel, M, N, K, epi, cap=0, ldc=None, note=""):
    """Bias + GELU forwards: gemm_ps 2 (c = pre, c2 = gelu), 5 (c = gelu', c2 = gelu), gemm_nt 2."""
    assert _supported(C, kernel, M, N, K, epi)
    op = _gelu_ops(M, N, K)
    a, b, bg = go.operand(op.A, gpu), go.operand(op.B, gpu), go.operand(op.bias[None, :], gpu)[0]
    pre = go.bf(op.exact + op.bias)  # gemm_ps.hip:330 / gemm.hip:290: the pre-activation as bf16 (exact: integers <= 8)
    out, c2 = go.output((M, N), gpu, ld=ldc), go.output((M, N), gpu, ld=ldc)
    _launch(C, kernel, a, b, out.view, c2.view, bg, None, epi, cap)
    case = f"M{M} N{N} K{K} cap{cap} epi{epi} gelu{note}"
    act64, act32 = go.gelu_tanh(pre), go.gelu_tanh(pre.float())
    go.assert_within(c2.result(), act64, go.allowance(act64, act32), kernel, case + " gelu")
    if epi == 5:
        g64, g32 = go.gelu_tanh_grad(pre), go.gelu_tanh_grad(pre.float())
        go.assert_within(out.result(), g64, go.allowance(g64, g32), kernel, case + " gelu'")
    else:
        go.assert_bits(out.result(), go.to_bf16(pre), kernel, case + " pre")
    assert out.border_intact() and c2.border_intact(), f"{kernel} {case}: wrote outside its outputs"


def _epi_dgelu(C, gpu, kernel, M, N, K, cap=0, ldc=None, note=""):
    """c = (a b^T) gelu'(c2) with fp32 column sums: gemm_ps 4, gemm_nt 3. c2: multiples of 1/8 in [-8, 8]."""
    epi = 4 if kernel == "gemm_ps" else 3
    assert _supported(C, kernel, M, N, K, epi)
    op = _ops("small", M, N, K)
    pre = torch.randint(-64, 65, (M, N), generator=torch.Generator().manual_seed(M + N + K)).double() / 8
    a, b = go.operand(op.A, gpu), go.operand(op.B, gpu)
    out, c2, cs = go.output((M, N), gpu, ld=ldc), go.output((M, N), gpu, ld=ldc, base=pre), go.GuardedF32(N, gpu)
    _launch(C, kernel, a, b, out.view, c2.view, None, cs.view, epi, cap)
    case = f"M{M} N{N} K{K} cap{cap} epi{epi} dgelu{note}"
    # gemm_ps.hip:330 rounds acc to bf16 before the multiply (:388); gemm.hip:274 multiplies the fp32 acc
    g = go.bf(op.exact) if kernel == "gemm_ps" else op.exact
    d64, d32 = g * go.gelu_tanh_grad(pre), g.float() * go.gelu_tanh_grad(pre.float())
    allow = go.allowance(d64, d32)
    go.assert_within(out.result(), d64, allow, kernel, case)
    # the column sums add the fp32 products (gemm_ps.hip:389) / the rounded bf16 products (gemm.hip:276)
    summand = go.allowance(d64, d32, final_rounding=kernel == "gemm_nt")
    cs_allow = summand.sum(0) + M * 2.0 ** -24 * d64.abs().sum(0)
    go.assert_within(cs.result(), d64.sum(0), cs_allow, kernel, case + " colsum")
    assert out.border_intact() and cs.border_intact() and c2.border_intact(), f"{kernel} {case}: wrote outside"
    assert torch.equal(c2.result().view(go.I16), go.to_bf16(pre).view(go.I16)), f"{kernel} {case}: c2 changed"


@pytest.mark.parametrize("M,N,K,cap", PS_SHAPES)
def test_gemm_ps_exact(C, gpu, M, N, K, cap):
    for fam in _families(K):
        op = _ops(fam, M, N, K)
        for epi in (0, 1):
            _epi_exact(C, gpu, "gemm_ps", op, epi, cap)
    _epi_exact(C, gpu, "gemm_ps", _ops("small", M, N, K), 6, cap)


@pytest.mark.parametrize("M,N,K,cap", PS_SHAPES)
def test_gemm_ps_gelu_epilogues(C, gpu, M, N, K, cap):
    for epi in (2, 5):
        _epi_gelu(C, gpu, "gemm_ps", M, N, K, epi, cap)
    _epi_dgelu(C, gpu, "gemm_ps", M, N, K, cap)


@pytest.mark.parametrize("M,N,K,cap", [PS_SHAPES[2], PS_SHAPES[3]])
def test_gemm_ps_onehot_and_slices(C, gpu, M, N, K, cap):
    _epi_exact(C, gpu, "gemm_ps", _ops("onehot", M, N, K), 0, cap)
    for live in go.live_slices(K // 32):
        _epi_exact(C, gpu, "gemm_ps", _ops("slice", M, N, K, live), 1, cap)


def test_gemm_ps_strided_rows(C, gpu):
    M, N, K, cap = PS_SHAPES[4]
    op = _ops("small", M, N, K)
    for epi in (0, 1, 6):
        _epi_exact(C, gpu, "gemm_ps", op, epi, cap, lda=K + 64, note=" lda")
        _epi_exact(C, gpu, "gemm_ps", op, epi, cap, ldc=N + 64, note=" ldc")
    _epi_gelu(C, gpu, "gemm_ps", M, N, K, 2, cap, ldc=N + 64, note=" ldc")
    _epi_gelu(C, gpu, "gemm_ps", M, N, K, 5, cap, ldc=N + 64, note=" ldc")
    _epi_dgelu(C, gpu, "gemm_ps", M, N, K, cap, ldc=N + 64, note=" ldc")


def test_gemm_ps_three_runs_equal_the_truth(C, gpu):
    M, N, K, cap = PS_SHAPES[3]
    for epi in (1, 6):
        _epi_exact(C, gpu, "gemm_ps", _ops("small", M, N, K), epi, cap, note=" x3", repeats=3)


NT_SHAPES = [(256, 256, 128),   # the shortest K
             (512, 256, 192), (512, 768, 256)]


@pytest.mark.parametrize("M,N,K", NT_SHAPES + [(300, 256, 192), (1300, 512, 128)])
def test_gemm_nt_exact(C, gpu, M, N, K):
    """Epilogues 0, 1 and 4 (bias + ReLU); they also take a ragged M (1300: 6 row panels, grouped_tile's last
    group of 2)."""
    for fam in _families(K):
        op = _ops(fam, M, N, K)
        for epi in (0, 1, 4):
            _epi_exact(C, gpu, "gemm_nt", op, epi)
    _epi_exact(C, gpu, "gemm_nt", _ops("onehot", M, N, K), 0)
    for live in go.live_slices(K // 32):
        _epi_exact(C, gpu, "gemm_nt", _ops("slice", M, N, K, live), 1)


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_gelu_epilogues(C, gpu, M, N, K):
    _epi_gelu(C, gpu, "gemm_nt", M, N, K, 2)
    _epi_dgelu(C, gpu, "gemm_nt", M, N, K)


def test_gemm_nt_three_runs_equal_the_truth(C, gpu):
    _epi_exact(C, gpu, "gemm_nt", _ops("small", 512, 768, 256), 1, note=" x3", repeats=3)
