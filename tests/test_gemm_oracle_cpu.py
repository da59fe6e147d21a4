"""The GEMM oracle (tests/_gemm_oracle.py) and the checks of tests/test_gemm_oracle_gpu.py proven sharp without a GPU.

`Emu` is a torch emulation of each kernel's dataflow behind the extension's own call signatures -- token / K splits
with fp32 partials, the split sum, accumulate, bias, the ragged panel, the 3x3 gather with zero padding, the epilogues
with their bf16 roundings -- into which one fault at a time can be injected. The GPU file's own case runners are run
against it: the clean emulation must pass every family bit-exact, and every mutant must be flagged on the family named
for it. The last test records why the oracle exists: the wrong kernels of the issue's table pass the old
`8e-3 * max|ref|` criterion."""
import pytest
import torch

from tests import _gemm_oracle as go
from tests import test_gemm_oracle_gpu as gt

CPU = torch.device("cpu")
FLAGGED = "differ from the exact result|outside the allowance|wrote outside"


@pytest.fixture(autouse=True)
def _no_report(monkeypatch):
    monkeypatch.delenv("GEMM_ORACLE_REPORT", raising=False)


def _i32(x):
    return x.contiguous().view(torch.int32)


def patch_matrix(x, stride, flip=False, fault=None):
    """[tokens, 9, Cin] fp32: the 3x3 patches (pad 1) of NHWC x as the kernels gather them, tap (ky, kx) of output
    pixel (img, oy, ox) = x[img, oy st + ky - 1, ox st + kx - 1] or 0 outside the image."""
    imgs, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    tok = torch.arange(imgs * Ho * Wo)
    img, rem = tok // (Ho * Wo), tok % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    flat = x.float().reshape(-1, Cc)
    out = torch.zeros(tok.numel(), 9, Cc)
    for t in range(9):
        ky, kx = divmod(t, 3)
        if flip and fault != "flip_not_flipped":
            ky, kx = 2 - ky, 2 - kx
        iy, ix = oy * stride + ky - 1, ox * stride + kx - 1
        if fault == "stride2_off_by_one" and stride == 2:
            ix = ix + 1
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        lin = (img * H + iy) * W + ix
        if fault == "left_border_wraps":  # ix = -1 read as the previous row's last pixel: no bounds check on x alone
            ok = ok | ((ix == -1) & (iy >= 0) & (iy < H) & (lin >= 0))
        if fault == "corner_padding" and t == 8:  # the last pixel's bottom-right tap reads the clamped pixel
            last = tok == tok.numel() - 1
            ok = ok | last
            lin = torch.where(last, torch.full_like(lin, flat.shape[0] - 1), lin)
        out[:, t] = torch.where(ok[:, None], flat[lin.clamp(0, flat.shape[0] - 1)], torch.zeros(()))
    return out


def _gelu32(x):
    return go.gelu_tanh(x.float())


class Emu:
    """The extension's GEMM entry points in torch on the CPU; `fault` plants one bug (sites in **site)."""

    def __init__(self, fault=None, **site):
        self.fault, self.site = fault, site

    # ---- the pieces every kernel shares
    def _round(self, x32):
        if self.fault == "truncate":
            return (_i32(x32.float()) & -65536).view(torch.float32).to(torch.bfloat16)
        return x32.float().to(torch.bfloat16)

    def _core(self, A, B, ranges):
        """sum over the K ranges of fp32 partials A[:, k0:k1] B[:, k0:k1]^T."""
        A, B = A.float().clone(), B.float()
        f, st = self.fault, self.site
        R = A.shape[0]
        if f == "lost_bit":
            A = (_i32(A) & ~0x10000).view(torch.float32)
        if f == "swap_rows":
            k1, k2 = st.get("k", (1, 2))
            A[:, [k1, k2]] = A[:, [k2, k1]]
        if f == "chunk_neighbour":
            r, k = st.get("rk", (8, 8))
            if st.get("along_rows"):  # gemm_wg: a 16-B chunk is 8 output rows of one token
                A[r:r + 8, k] = A[r + 8:r + 16, k].clone()
            else:
                A[r, k:k + 8] = A[r, k + 8:k + 16].clone()
        if f == "ragged_clamp":  # the clamp of the half panel's last chunk lands one chunk early
            A[R - 8:R] = A[R - 16:R - 8].clone()
        ranges = [list(r) for r in ranges]
        if f == "split_block_twice" and len(ranges) > 1:
            ranges[0][1] += 64
        if f == "split_block_missed" and len(ranges) > 1:
            ranges[1][0] += 64
        parts = []
        for i, (k0, k1) in enumerate(ranges):
            p = A[:, k0:k1] @ B[:, k0:k1].t()
            if f == "stale_slot" and i == st.get("split", 0):  # slice s + 4 of one tile still holds slice s
                lo = k0 + 32 * st.get("slice", 0)
                p[:256, :256] += (A[:256, lo:lo + 32] @ B[:256, lo:lo + 32].t()
                                  - A[:256, lo + 128:lo + 160] @ B[:256, lo + 128:lo + 160].t())
            if f == "partials_bf16":
                p = p.to(torch.bfloat16).float()
            parts.append(p)
        if f == "missing_partial" and len(parts) > 1:
            parts.pop()
        total = parts[0]
        for p in parts[1:]:
            total = total + p
        if f == "drop_token":  # one k (a token of gemm_wg) missing from one output row
            r = st.get("r", 5)
            k = int(A[r].abs().argmax())
            total[r] -= A[r, k] * B[:, k]
        return total

    def _finish(self, total, bias=None, base=None):
        if bias is not None:
            if self.fault == "bias_after_rounding":
                return self._round(self._round(total).float() + bias.float())
            total = total + bias.float()
        if base is not None:
            if self.fault == "acc_ignores_base":
                return self._round(total)
            if self.fault == "acc_rounds_twice":
                return self._round(base.float() + self._round(total).float())
            total = base.float() + total
        return self._round(total)

    # ---- gemm_wg.hip
    @staticmethod
    def _wg_ranges(K, splits):
        nb = K // 64
        return [(64 * (s * nb // splits), 64 * ((s + 1) * nb // splits)) for s in range(splits)]

    @staticmethod
    def _wg_splits(M, N, K):
        tiles = ((M + 255) // 256) * ((N + 255) // 256)
        return max(1, min(256 // tiles, K // 768))

    def gemm_wg_supported(self, M, N, K, splits=0):
        splits = splits if splits > 0 else self._wg_splits(M, N, K)
        return M % 128 == 0 and N % 256 == 0 and K % 64 == 0 and K // 192 >= splits

    def gemm_wg(self, a, b, out, accumulate=False, splits=0, loaders=8):
        K, M, N = a.shape[0], a.shape[1], b.shape[1]
        splits = splits if splits > 0 else self._wg_splits(M, N, K)
        total = self._core(a.t(), b.t(), self._wg_ranges(K, splits))
        out.copy_(self._finish(total, base=out.clone() if accumulate else None))

    def gemm_wg_conv3x3_supported(self, Cout, Cin, imgs, H, W, stride):
        return True

    def gemm_wg_conv3x3(self, dy, x, out, accumulate=False, stride=1, splits=0):
        cout, cin = dy.shape[3], x.shape[3]
        P = patch_matrix(x, stride, fault=self.fault).reshape(-1, 9 * cin)
        T = P.shape[0]
        splits = splits if splits > 0 else self._wg_splits(cout, 9 * cin, T)
        total = self._core(dy.reshape(T, cout).t(), P.t(), self._wg_ranges(T, splits))
        out.copy_(self._finish(total, base=out.clone() if accumulate else None))

    # ---- gemm_f.hip
    def gemm_f_supported(self, M, N, K):
        return (N % 128 == 0 or N == 64) and K % 64 == 0 and K >= 192

    @staticmethod
    def _f_split_ok(K, s):
        nk = K // 32
        return 1 <= s <= 16 and nk % s == 0 and (nk // s) % 2 == 0 and nk // s >= 6

    def gemm_f_splits(self, M, N, K):
        bn = 64 if N <= 64 else 128 if N <= 128 else 256
        tiles = ((M + 255) // 256) * ((N + bn - 1) // bn)
        best = 1
        for s in range(2, 17):
            if tiles * s <= 256 and self._f_split_ok(K, s):
                best = s
        return best

    def _f(self, A, B, out, bias, splits, M, N, K):
        splits = self.gemm_f_splits(M, N, K) if splits < 0 else max(splits, 1)
        assert self._f_split_ok(K, splits) or splits == 1
        per = K // splits
        total = self._core(A, B, [(s * per, (s + 1) * per) for s in range(splits)])
        out.copy_(self._finish(total, bias=bias).reshape(out.shape))

    def gemm_f(self, a, b, out, bias=None, waves=0, splits=-1):
        self._f(a, b, out, bias, splits, a.shape[0], b.shape[0], a.shape[1])

    def gemm_f_conv3x3_supported(self, imgs, H, W, Cin, Cout, stride):
        return True

    def gemm_f_conv3x3(self, x, w, out, stride, bias=None, waves=0, splits=-1, flip_taps=False):
        cin = x.shape[3]
        if w.dim() == 3 and self.fault != "tap_major_as_channel_major":
            cout = w.shape[1]
            B = w.permute(1, 0, 2).reshape(cout, 9 * cin)
        else:  # [Cout][ky][kx][Cin] rows (the fault: a tap-major w read as if it were that)
            cout = w.shape[1] if w.dim() == 3 else w.shape[0]
            B = w.reshape(cout, 9 * cin)
        P = patch_matrix(x, stride, flip=flip_taps, fault=self.fault).reshape(-1, 9 * cin)
        self._f(P, B, out, bias, splits, P.shape[0], cout, 9 * cin)

    # ---- gemm_ps.hip / gemm.hip
    def gemm_ps_supported(self, M, N, K, epi):
        return M % 256 == 0 and N % 256 == 0 and K % 128 == 0 and K >= 256 and epi in (0, 1, 2, 4, 5, 6)

    def gemm_nt_supported_epi(self, M, N, K, epi):
        return N % 256 == 0 and K % 64 == 0 and K >= 128 and (epi in (0, 1, 4) or (epi in (2, 3) and M % 256 == 0))

    def _colsum(self, d, colsum):
        if self.fault == "colsum_missing_row":
            d = d[:-1]
        colsum += d.float().sum(0)

    def gemm_ps(self, a, b, c, c2=None, bias=None, colsum=None, epi=0, grid_cap=0):
        acc = self._core(a, b, [(0, a.shape[1])])
        v = self._finish(acc, bias=bias if epi in (1, 2, 5) else None)  # gemm_ps.hip:330
        if epi in (0, 1):
            c.copy_(v)
        elif epi == 2:
            c.copy_(v)
            c2.copy_(self._round(_gelu32(v)))
        elif epi == 5:
            c.copy_(self._round(go.gelu_tanh_grad(v.float())))
            c2.copy_(self._round(_gelu32(v)))
        else:
            d = v.float() * (c2.float() if epi == 6 else go.gelu_tanh_grad(c2.float()))
            c.copy_(self._round(d))
            self._colsum(d, colsum)

    def gemm_nt(self, a, b, c, c2=None, bias=None, colsum=None, epi=0):
        acc = self._core(a, b, [(0, a.shape[1])])
        if epi == 3:
            d = self._round(acc * go.gelu_tanh_grad(c2.float()))  # gemm.hip:274
            c.copy_(d)
            self._colsum(d, colsum)  # :276
            return
        v = self._finish(acc, bias=bias if epi in (1, 2, 4) else None)
        c.copy_(v.float().clamp_min(0.0).to(torch.bfloat16) if epi == 4 else v)
        if epi == 2:
            c2.copy_(self._round(_gelu32(v)))


# ------------------------------------------------------------------------------------ the clean emulation passes
def test_clean_emulation_is_bit_exact_on_every_family():
    E = Emu()
    for K, M, N, s in [(448, 256, 256, 2), (192, 128, 256, 1), (384, 384, 512, 2)]:
        for fam in ("small", "mantissa", "onehot"):
            for acc in (False, True):
                gt._wg_run(E, CPU, gt._ops(fam, M, N, K), s, 8, acc, lda=M + 64)
        for live in go.live_slices(K // 32, s):
            gt._wg_run(E, CPU, gt._ops("slice", M, N, K, live), s, 8, False)
    for M, N, K, s in [(300, 384, 256, -2), (300, 384, 768, 4), (1, 64, 192, -2)]:
        for fam in ("small", "mantissa", "onehot"):
            gt._f_run(E, CPU, gt._ops(fam, M, N, K), 8, True, splits=s, ldc=N + 64)
        gt._f_run(E, CPU, gt._ops("slice", M, N, K, K // 32 - 1), 8, True, splits=s)
    for shape, s in [(gt.WGC_SHAPES[0][:6], 1), (gt.WGC_SHAPES[3][:6], 1), (gt.WGC_SHAPES[5][:6], 2)]:
        for fam in ("small", "mantissa", "onehot"):
            gt._wgc_run(E, CPU, fam, shape, s, fam == "small")
        gt._wgc_run(E, CPU, "slice", shape, s, False, live=5)
    for shape in (gt.FC_SHAPES[0], gt.FC_SHAPES[3], gt.FC_SHAPES[4], (2, 5, 4, 64, 128, 1)):
        for fam in ("small", "mantissa", "onehot"):
            for mode in gt.FC_MODES:
                gt._fc_run(E, CPU, fam, shape, mode, 8, fam != "onehot")
    for kernel, (M, N, K) in (("gemm_ps", (256, 256, 256)), ("gemm_nt", (256, 256, 128)), ("gemm_nt", (300, 256, 192))):
        for fam in ("small", "mantissa", "onehot"):
            for epi in (0, 1) + ((6,) if kernel == "gemm_ps" and fam == "small" else ()):
                gt._epi_exact(E, CPU, kernel, gt._ops(fam, M, N, K), epi)
        if M % 256 == 0:
            for epi in ((2, 5) if kernel == "gemm_ps" else (2,)):
                gt._epi_gelu(E, CPU, kernel, M, N, K, epi)
            gt._epi_dgelu(E, CPU, kernel, M, N, K)
    gt._epi_exact(E, CPU, "gemm_nt", gt._ops("small", 300, 256, 192), 4)


def test_guard_bands_and_prefill_are_checked():
    """An unwritten element (the NaN pre-fill), a store past the view and a read of the NaN border all show."""
    class Lazy(Emu):  # leaves the last output row unwritten
        def gemm_f(self, a, b, out, bias=None, waves=0, splits=-1):
            tmp = torch.empty(out.shape, dtype=out.dtype)
            Emu.gemm_f(self, a, b, tmp, bias, waves, splits)
            out[:-1].copy_(tmp[:-1])

    class Spill(Emu):  # also writes the gap column after the view
        def gemm_f(self, a, b, out, bias=None, waves=0, splits=-1):
            Emu.gemm_f(self, a, b, out, bias, waves, splits)
            out.as_strided((out.shape[0], out.shape[1] + 1), out.stride())[:, -1] = 0

    class Overread(Emu):  # reads one row past a ragged operand
        def gemm_f(self, a, b, out, bias=None, waves=0, splits=-1):
            a2 = a.as_strided((a.shape[0] + 1, a.shape[1]), a.stride())
            tmp = torch.empty(out.shape[0] + 1, out.shape[1], dtype=out.dtype)
            Emu.gemm_f(self, a2, b, tmp, bias, waves, splits)
            out.copy_(tmp[:-1] + tmp[-1:] * 0)

    op = gt._ops("small", 300, 384, 256)
    for bad in (Lazy(), Spill(), Overread()):
        with pytest.raises(AssertionError, match=FLAGGED):
            gt._f_run(bad, CPU, op, 8, False, ldc=384 + 64)


# ------------------------------------------------------------------------------------ every mutant is flagged
WG = (448, 256, 256, 2)  # (K, M, N, splits)


def _wg(E, fam, acc=False, shape=WG, live=None):
    K, M, N, s = shape
    gt._wg_run(E, CPU, gt._ops(fam, M, N, K, live), s, 8, acc)


def _f(E, fam, shape=(300, 384, 768), splits=4, live=None):
    gt._f_run(E, CPU, gt._ops(fam, *shape, live), 8, True, splits=splits)


MUTANTS = [
    ("truncate", {}, lambda E: _wg(E, "mantissa")),
    ("truncate", {}, lambda E: _f(E, "mantissa")),
    ("partials_bf16", {}, lambda E: _wg(E, "mantissa")),
    ("partials_bf16", {}, lambda E: _f(E, "mantissa")),
    ("lost_bit", {}, lambda E: _wg(E, "mantissa")),
    ("drop_token", {}, lambda E: _wg(E, "small")),
    ("drop_token", {}, lambda E: _wg(E, "onehot")),
    ("swap_rows", {}, lambda E: _wg(E, "small")),
    ("swap_rows", {}, lambda E: _f(E, "small")),
    ("chunk_neighbour", {"along_rows": True}, lambda E: _wg(E, "small")),
    ("chunk_neighbour", {"rk": (5, 64)}, lambda E: _f(E, "small")),
    ("stale_slot", {"split": 0, "slice": 1}, lambda E: _wg(E, "slice", live=5)),   # slice 5 never arrives
    ("stale_slot", {"split": 0, "slice": 1}, lambda E: _wg(E, "slice", live=1)),   # slice 1 counted twice
    ("stale_slot", {"split": 1, "slice": 0}, lambda E: _f(E, "slice", live=10)),
    ("split_block_twice", {}, lambda E: _wg(E, "small")),
    ("split_block_twice", {}, lambda E: _wg(E, "slice", live=6)),    # split 1's first slice (blocks 0-2 | 3-6)
    ("split_block_missed", {}, lambda E: _wg(E, "small")),
    ("split_block_missed", {}, lambda E: _wg(E, "slice", live=7)),
    ("missing_partial", {}, lambda E: _wg(E, "small")),
    ("missing_partial", {}, lambda E: _f(E, "small")),
    ("acc_ignores_base", {}, lambda E: _wg(E, "small", acc=True)),
    ("acc_rounds_twice", {}, lambda E: _wg(E, "mantissa", acc=True)),
    ("bias_after_rounding", {}, lambda E: _f(E, "mantissa")),
    ("bias_after_rounding", {}, lambda E: gt._epi_exact(E, CPU, "gemm_ps", gt._ops("mantissa", 256, 256, 256), 1)),
    ("colsum_missing_row", {}, lambda E: gt._epi_exact(E, CPU, "gemm_ps", gt._ops("small", 256, 256, 256), 6)),
    ("colsum_missing_row", {}, lambda E: gt._epi_dgelu(E, CPU, "gemm_ps", 256, 256, 256)),
    ("ragged_clamp", {}, lambda E: _wg(E, "small", shape=(192, 128, 256, 1))),
    ("ragged_clamp", {}, lambda E: _wg(E, "onehot", shape=(384, 384, 512, 2))),
    ("left_border_wraps", {}, lambda E: gt._fc_run(E, CPU, "onehot", gt.FC_SHAPES[3], "plain", 8, False)),
    ("left_border_wraps", {}, lambda E: gt._wgc_run(E, CPU, "onehot", gt.WGC_SHAPES[0][:6], 1, False)),
    ("corner_padding", {}, lambda E: gt._fc_run(E, CPU, "small", gt.FC_SHAPES[1], "plain", 8, False)),
    ("corner_padding", {}, lambda E: gt._wgc_run(E, CPU, "small", gt.WGC_SHAPES[1][:6], 1, False)),
    ("stride2_off_by_one", {}, lambda E: gt._fc_run(E, CPU, "small", gt.FC_SHAPES[4], "plain", 8, False)),
    ("stride2_off_by_one", {}, lambda E: gt._wgc_run(E, CPU, "small", gt.WGC_SHAPES[3][:6], 1, False)),
    ("flip_not_flipped", {}, lambda E: gt._fc_run(E, CPU, "small", gt.FC_SHAPES[1], "flip", 8, False)),
    ("tap_major_as_channel_major", {}, lambda E: gt._fc_run(E, CPU, "small", gt.FC_SHAPES[1], "tapmajor", 8, False)),
]


@pytest.mark.parametrize("i", range(len(MUTANTS)), ids=[f"{m[0]}-{i}" for i, m in enumerate(MUTANTS)])
def test_every_mutant_is_flagged(i):
    fault, site, run = MUTANTS[i]
    run(Emu())  # the same case passes clean ...
    with pytest.raises(AssertionError, match=FLAGGED):
        run(Emu(fault, **site))  # ... and the planted bug changes bits


def test_failure_message_names_tile_and_fetched_element():
    op = gt._ops("onehot", 384, 512, 384)
    h = int(op.hot[300])  # row 300's one-hot k: its 16-B chunk is replaced by (or copied over) the neighbouring one
    with pytest.raises(AssertionError) as e:
        gt._wg_run(Emu("chunk_neighbour", rk=(300, h - h % 16)), CPU, op, 2, 8, False)
    msg = str(e.value)
    assert "gemm_wg" in msg and "(1, 0)" in msg and "fetched B[" in msg and "got" in msg and "want" in msg


# ------------------------------------------------------------------------------------ why the oracle exists
@pytest.mark.parametrize("K,M,N,splits,passing", [
    (8192, 2304, 768, 9, ("truncate", "partials_bf16", "lost_bit", "drop_token", "acc_rounds_twice")),
    (65536, 768, 768, 28, ("truncate", "partials_bf16", "lost_bit", "drop_token", "chunk_neighbour", "acc_rounds_twice"))])
def test_old_criterion_lets_the_mutants_through(K, M, N, splits, passing):
    """The criterion of test_gemm_wg_matches_fp32 -- randn operands, max|out - ref| <= 8e-3 max|ref| -- accepts these
    wrong kernels (five at 8192 tokens, all six at 65536; the misread chunk is caught at 8192 only because ITS size does
    not grow with the token count while the allowance does)."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(K, M, generator=g).to(torch.bfloat16).float()
    b = torch.randn(K, N, generator=g).to(torch.bfloat16).float()
    base = torch.randn(M, N, generator=g).to(torch.bfloat16).float()
    E = Emu()
    parts = [a[k0:k1].t() @ b[k0:k1] for k0, k1 in E._wg_ranges(K, splits)]
    total = sum(parts[1:], parts[0])
    ref = a.t() @ b
    tol = 8e-3 * float(ref.abs().max())

    def err(out, want=ref):
        return float((out.float() - want).abs().max())

    assert err(total.to(torch.bfloat16)) <= tol  # the clean kernel
    trunc = Emu("truncate")
    lost = (_i32(a) & ~0x10000).view(torch.float32)
    k0, m0 = K // 3 + 1, 37
    # the misread chunk at the token where it costs least (its error is |delta a| |b| of ONE token, whatever K is):
    # such a fault need only exist to show the criterion blind to it
    kc = int(((a[:, 72:80] - a[:, 64:72]).abs().amax(1) * b.abs().amax(1)).argmin())
    chunk = total.clone()
    chunk[64:72] += (a[kc, 72:80] - a[kc, 64:72])[:, None] * b[kc][None, :]
    dropped = total.clone()
    dropped[m0] -= a[k0, m0] * b[k0]
    errs = {"truncate": err(trunc._round(total)),
            "partials_bf16": err(sum((p.to(torch.bfloat16).float() for p in parts[1:]), parts[0].to(torch.bfloat16).float())
                                 .to(torch.bfloat16)),
            "lost_bit": err((lost.t() @ b).to(torch.bfloat16)),
            "drop_token": err(dropped.to(torch.bfloat16)),
            "chunk_neighbour": err(chunk.to(torch.bfloat16)),
            "acc_rounds_twice": err((base + total.to(torch.bfloat16).float()).to(torch.bfloat16), ref + base)}
    for name in passing:
        assert errs[name] <= tol, (name, errs[name], tol)
    # ... while each of them changes bits of an exact family at the smallest shapes (test_every_mutant_is_flagged)
