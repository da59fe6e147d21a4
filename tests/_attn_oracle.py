"""Per-tile oracle for the causal attention kernels (attention.hip, attention_hm.hip).

Three pieces, all plain torch and importable without a GPU:

  reference       float64 causal (GQA-aware) attention: o, lse (natural log), dq, dk, dv
  rounding_model  fp32 emulation of the same mathematics that rounds to bf16 exactly where the
                  named kernel does (every rounding cites the source line it was read from)
  check           per (batch, head, 32 consecutive rows): |got - ref| <= K |model - ref| + floor

K and the floor are fixed by reasoning about the number formats and are NOT tuned to make a
kernel pass:

  K = 4      the model and a kernel share their rounding points; what differs is the fp32
             accumulation order and the 1-ulp hardware exp2 (both far below 2^-9, the bf16 unit
             roundoff) and that the two are independent draws of the same rounding noise, whose
             per-tile norm ratio scatters up to about 2x. 4 leaves 2x over that scatter.
  floor      2^-10 |ref[b, h]|_F / sqrt(ntiles): about 0.1 % of an average tile of that head.
             Needed because reference tiles legitimately shrink to ~1e-24 (dK / dV of keys that
             nobody attends to in the descending-ladder family).

Measured (profiles/attention_oracle_ratios.txt): the shipped kernels sit at 0.9 - 1.1x the model's
error on every family, because they round the same fp32 values as the model far more often than
two independent draws would. A kernel with another evaluation order (say a 32-key tile) is a truly
independent draw; on a ragged tile of ONE row, where a single rounding (that row's delta) can
dominate, the ratio of two draws has a heavy tail and has been seen at 4.3x in the CPU model
(wide3, D = 128, T = 65). Such a finding is to be read from the tile it names, not tuned away.

All tensors here are head-major: q, do, o, dq [B, Hq, T, D]; k, v, dk, dv [B, Hkv, T, D];
lse [B, Hq, T]. pack_qkv / unpack_dqkv / token_major adapt to the packed [B, T, 3, H, 64] and the
token-major [B, T, H, D] layouts of the kernels.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
K_BOUND = 4.0
FLOOR = 2.0 ** -10
WAVE_ROWS = 32            # one wave's share of the rows in the forward, dQ and dK/dV kernels alike
KEY_TILE = 64             # attn_common.h:17 A_BK, keys per LDS tile = granularity of the running max
RESCALE_THRESHOLD = 8.0   # attention.hip:125 / :314, attention_hm.hip:87

FAMILIES = ("randn", "wide3", "up5", "up12", "down12")
_LADDER = {"up5": 5.0, "up12": 12.0, "down12": -12.0}  # log2 units per 64-key tile


# ------------------------------------------------------------------------------------ inputs
def score_scale_log2(scale: float) -> float:
    """c = scale * log2 e as the launchers compute it: an fp32 product (attention.hip:1194)."""
    return float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def make_inputs(family, B, Hq, Hkv, T, D, scale, seed=0, device="cpu"):
    """Seeded bf16 q, k, v, do (head-major). Drawn on the CPU so every device sees the same values.

    randn    unit normal (the inputs of tests/test_attention_gpu.py)
    wide3    q and k times 3: log2-domain score std ~13, row ranges ~100 -> real rescales,
             underflowing tiles, and the dQ kernels' prescale rounding made visible
    up5 / up12 / down12
             randn plus a rank-one ladder q += 8 u, k_j += (delta * floor(j / 64) / (8 c)) u with u
             a fixed unit vector: the running max moves by ~delta (log2 units) per key tile.
             up5: below the 2^8 threshold every tile, so the stale-max branch alternates with real
             rescales; up12: a rescale at every tile; down12: the max sits in the first tile, no
             rescale after it, later tiles underflow to 0. Keep T <= 452 (k stays below ~60).
    """
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(B, Hq, T, D, generator=g)
    k = torch.randn(B, Hkv, T, D, generator=g)
    v = torch.randn(B, Hkv, T, D, generator=g)
    do = torch.randn(B, Hq, T, D, generator=g)
    if family == "wide3":
        q, k = q * 3, k * 3
    elif family in _LADDER:
        u = torch.randn(D, generator=torch.Generator(device="cpu").manual_seed(977))
        u = u / u.norm()
        c = scale * LOG2E
        step = torch.div(torch.arange(T), KEY_TILE, rounding_mode="floor").to(torch.float32)
        q = q + 8.0 * u
        k = k + (_LADDER[family] * step / (8.0 * c))[:, None] * u
    elif family != "randn":
        raise ValueError(family)
    return tuple(t.to(torch.bfloat16).to(device) for t in (q, k, v, do))


def pack_qkv(q, k, v):
    """Head-major q, k, v (Hq == Hkv) -> packed [B, T, 3, H, D] (attention.hip layout)."""
    return torch.stack((q, k, v), 0).permute(1, 3, 0, 2, 4).contiguous()


def unpack_dqkv(dqkv):
    """Packed [B, T, 3, H, D] -> head-major dq, dk, dv views."""
    return dqkv.permute(2, 0, 3, 1, 4).unbind(0)


def token_major(x):
    """[B, H, T, D] <-> [B, T, H, D] (o and do of both kernels are token-major), contiguous."""
    return x.transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------ reference
def _group_sum(x, Hkv):
    B, Hq, T, D = x.shape
    return x.view(B, Hkv, Hq // Hkv, T, D).sum(2)


def reference(q, k, v, do, scale):
    """float64 causal attention and its gradients for the upstream gradient do."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    Hq, Hkv, T = q.shape[1], k.shape[1], q.shape[2]
    rep = Hq // Hkv
    kx, vx = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    masked = torch.triu(torch.ones(T, T, dtype=torch.bool, device=q.device), 1)
    s = (q @ kx.transpose(-1, -2) * scale).masked_fill(masked, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = p @ vx
    dp = do @ vx.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    # dS = P (dP - delta) cancels (exactly, to dq = dk = 0, on a row with a single key): the size of the
    # terms that cancel, |P| (|dP| + |delta|) carried through the same products, is what an fp32
    # evaluation's roundoff scales with (check()'s `mag`)
    a = p * (dp.abs() + delta.abs())
    return {"o": o, "lse": lse, "dq": ds @ kx * scale,
            "dk": _group_sum(ds.transpose(-1, -2) @ q * scale, Hkv),
            "dv": _group_sum(p.transpose(-1, -2) @ do, Hkv),
            "dq_mag": a @ kx.abs() * scale, "dk_mag": _group_sum(a.transpose(-1, -2) @ q.abs() * scale, Hkv)}


def reference_packed(qkv, do_tm, scale):
    """reference() for the packed layout: qkv [B, T, 3, H, D], do_tm [B, T, H, D] (token-major)."""
    q, k, v = unpack_dqkv(qkv)
    return reference(q, k, v, do_tm.transpose(1, 2), scale)


# ------------------------------------------------------------------------------------ rounding model
KERNELS = ("d64", "hm")  # attention.hip (packed, D = 64) / attention_hm.hip (head-major GQA, D = 64 / 128)


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def rounding_model(q, k, v, do, scale, kernel, *, prescale=None, key_tile=KEY_TILE, acc=torch.float32,
                   fault=None):
    """fp32 emulation of `kernel` ("d64" or "hm") with its bf16 rounding points.

    Rounding points shared by both files (d64 line / hm line):
      forward   P -> bf16 before P V (attention.hip:153, :342 / attention_hm.hip:117); the row sum l
                adds the UNROUNDED fp32 p (:144-147 / :104-111); p is taken against the deferred
                (possibly stale, up to 2^8 low) running max of the wave's 32 rows (:125 / :87);
                O = acc / l -> bf16 (store_acc_tile, attn_common.h:163, called at :191 / :150);
                lse = m + log2 l in fp32, log2 domain (:193 / :153)
      dQ        delta = rowsum(dO * bf16 O) in fp32 (:447, :990 / :194); P recomputed against the
                forward's lse; dS -> bf16 (:512, :1049 / :240); dQ * scale -> bf16 (:550, :1094 / :274)
      dK / dV   P from fma(S, c, -lse) (:674, :853 / :376), P -> bf16 for dV (:688, :867 / :390),
                dS -> bf16 for dK (:689, :868 / :391); the GQA kernel sums a group's query heads in
                the fp32 accumulators, one bf16 rounding at the end (attention_hm.hip:433, :436);
                dK * scale and dV -> bf16 (:751-752, :948-949 / :433-436)
    Only in the d64 dQ kernels (attention.hip:455, :999; attn_common.h:59 prescale): the scores
    are recomputed from bf16(Q * c), one more rounding whose error grows with |score|.
    attention_hm.hip's dQ kernel (:229) and every dK/dV kernel use fma(S, c, -lse) on the raw bf16 Q.

    prescale   None: as the named kernel does; True / False: force (to put the cost on record)
    key_tile / acc   the evaluation order: a different key tile or accumulation type gives an
               independent draw of the same rounding noise (the oracle self-test's "second seed")
    fault      planted bugs for the oracle's self-test: "mask_off_by_one" (key >= q masked),
               "extra_key" (the last query also sees a clamped duplicate of key T - 1 at index T),
               "skip_rescale:<tile>" (O accumulator not multiplied by alpha at that key tile)
    Returns fp32 tensors holding bf16 values: o, dq, dk, dv; lse2 (log2 domain, as the kernels store
    it) and lse (natural log).
    """
    if kernel not in KERNELS:
        raise ValueError(kernel)
    if prescale is None:
        prescale = kernel == "d64"
    dev = q.device
    qf, kf, vf, dof = (t.to(torch.float32) for t in (q, k, v, do))
    B, Hq, T, D = qf.shape
    Hkv = kf.shape[1]
    rep = Hq // Hkv
    kx, vx = kf.repeat_interleave(rep, 1), vf.repeat_interleave(rep, 1)
    if fault == "extra_key":
        kx, vx = torch.cat((kx, kx[:, :, -1:]), 2), torch.cat((vx, vx[:, :, -1:]), 2)
    Tk = kx.shape[2]
    c = score_scale_log2(scale)
    scale32 = float(torch.tensor(scale, dtype=torch.float32))

    def mm(a, b):
        return (a.to(acc) @ b.to(acc)).to(torch.float32)

    qi = torch.arange(T, device=dev)[:, None]
    ki = torch.arange(Tk, device=dev)[None, :]
    masked = ki > qi - (1 if fault == "mask_off_by_one" else 0)
    if fault == "extra_key":
        masked[T - 1, T] = False
    skip_tile = int(fault.split(":")[1]) if fault and fault.startswith("skip_rescale:") else -1

    S = mm(qf, kx.transpose(-1, -2))  # raw scores, fp32 accumulation of bf16 products
    # ---- forward: online softmax over key tiles, rescale deferred per 32-row wave
    m = torch.full((B, Hq, T), float("-inf"), device=dev)
    l = torch.zeros(B, Hq, T, device=dev)
    o = torch.zeros(B, Hq, T, D, device=dev)
    for ti, kb in enumerate(range(0, Tk, key_tile)):
        if kb >= T:
            break
        ke = min(kb + key_tile, Tk)
        # a wave skips the tiles whose first key lies past its last row (attention.hip:102): rows kb..
        s = S[:, :, kb:, kb:ke].masked_fill(masked[kb:, kb:ke], float("-inf"))
        mx = s.amax(-1) * c  # :124 max of the raw scores, then * c
        mo = m[:, :, kb:]
        n = T - kb
        pad = -n % WAVE_ROWS
        need = F.pad((mx - mo) > RESCALE_THRESHOLD, (0, pad)).view(B, Hq, -1, WAVE_ROWS).any(-1, keepdim=True)
        need = need.expand(-1, -1, -1, WAVE_ROWS).reshape(B, Hq, -1)[:, :, :n]  # :125 __all over the wave
        mnew = torch.where(need, torch.maximum(mo, mx), mo)
        alpha = torch.exp2(mo - mnew)
        p = torch.exp2(s * c - mnew[..., None])  # :140 fma(s, c, -m)
        l[:, :, kb:] = l[:, :, kb:] * alpha + p.sum(-1)  # :128, :147 fp32 p
        oa = o[:, :, kb:] if ti == skip_tile else o[:, :, kb:] * alpha[..., None]
        o[:, :, kb:] = oa + mm(_bf(p), vx[:, :, kb:ke])  # :153 P -> bf16
        m[:, :, kb:] = mnew
    o_out = _bf(o * (1.0 / l)[..., None])  # :190-191 inv = 1 / l, bf16 store
    lse2 = m + torch.log2(l)  # :193

    # ---- backward
    delta = (o_out * dof).sum(-1, keepdim=True)  # :447 bf16 O times bf16 dO, fp32 sum
    dP = mm(dof, vx.transpose(-1, -2))
    if prescale:
        st = mm(_bf(qf * c), kx.transpose(-1, -2)) - lse2[..., None]  # :455 prescale, :493 lse as the initial accumulator
    else:
        st = S * c - lse2[..., None]  # attention_hm.hip:229
    ds = _bf(torch.exp2(st).masked_fill(masked, 0.0) * (dP - delta))  # :506, :512 dS -> bf16
    dq = _bf(mm(ds, kx) * scale32)  # :550
    p2 = torch.exp2(S * c - lse2[..., None]).masked_fill(masked, 0.0)  # :674 (no prescale in dK/dV)
    ds2 = _bf(p2 * (dP - delta))  # :680, :689
    dk = _bf(_group_sum(mm(ds2.transpose(-1, -2), qf)[:, :, :T], Hkv) * scale32)  # :751
    dv = _bf(_group_sum(mm(_bf(p2).transpose(-1, -2), dof)[:, :, :T], Hkv))  # :688, :752
    return {"o": o_out, "lse2": lse2, "lse": lse2 * LN2, "dq": dq, "dk": dk, "dv": dv}


# ------------------------------------------------------------------------------------ checks
def _tile_norms(x, rows):
    B, H, T, D = x.shape
    nt = (T + rows - 1) // rows
    x = F.pad(x, (0, 0, 0, nt * rows - T))
    return x.reshape(B, H, nt, rows * D).norm(dim=-1)


def check(got, ref, model, rows=WAVE_ROWS, K=K_BOUND, name="", strict=True, mag=None):
    """Per (batch, head, `rows` consecutive rows): |got - ref|_F <= K |model - ref|_F + floor, with
    floor = 2^-10 |ref[b, h]|_F / sqrt(ntiles). mag (dq, dk: reference()'s dq_mag / dk_mag) adds
    2^-21 |mag tile|_F to the floor: fp32 roundoff (2^-24, the 8x headroom of lse_tolerance) of the
    terms that cancel in dS. It is 2^-11 of the first term wherever the gradient is not itself a
    cancellation, and the whole floor where it is (T = 1: dq = dk = 0 exactly, so the first term is 0
    and any two fp32 summation orders would fail each other). No tile is skipped. Returns the worst ratio
    |got - ref| / (|model - ref| + floor / K), which the bound holds to K; a NaN or inf anywhere in
    `got` gives inf. strict: raise AssertionError naming the worst tile when the bound is exceeded."""
    g, r, mo = got.double(), ref.double(), model.double()
    assert g.shape == r.shape == mo.shape and r.dim() == 4, (g.shape, r.shape, mo.shape)
    eg, em = _tile_norms(g - r, rows), _tile_norms(mo - r, rows)
    nt = eg.shape[-1]
    floor = (FLOOR * r.flatten(2).norm(dim=-1, keepdim=True) / math.sqrt(nt)).expand_as(eg)
    if mag is not None:
        floor = floor + 2.0 ** -21 * _tile_norms(mag.double(), rows)
    ratio = eg / (em + floor / K)
    ratio = torch.where(eg == 0, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    if strict and not worst <= K:
        b, h, t = (int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise AssertionError(f"{name}: rows {t * rows}..{min((t + 1) * rows, r.shape[2]) - 1} of (b={b}, h={h}): "
                             f"error {float(eg[b, h, t]):.4g} is {worst:.3g}x the rounding model's "
                             f"{float(em[b, h, t]):.4g} (+ floor {float(floor[b, h, t]) / K:.3g}); bound {K}x")
    return worst


def lse_tolerance(q, k, scale):
    """Per row i: 2^-21 max_{j <= i}(|q_i| |k_j|) scale + 2^-18. The fp32 unit roundoff 2^-24 times the
    largest score magnitude the row can accumulate, with 8x headroom for accumulation order and the
    hardware exp2 / log2, plus the same headroom on an O(1) log-sum."""
    rep = q.shape[1] // k.shape[1]
    qn = q.double().norm(dim=-1)
    kn = k.double().norm(dim=-1).cummax(-1).values.repeat_interleave(rep, 1)
    return 2.0 ** -21 * qn * kn * scale + 2.0 ** -18


def lse_check(lse2, ref_lse, q, k, scale, name="", strict=True):
    """lse2: the kernel's log2-domain lse [B, Hq, T]; compares lse2 * ln 2 with the float64 reference
    per row. Returns the worst |error| / tolerance (must be <= 1)."""
    err = (lse2.double() * LN2 - ref_lse.double()).abs() / lse_tolerance(q, k, scale)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    worst = float(err.max())
    if strict and not worst <= 1.0:
        b, h, t = (int(i) for i in torch.unravel_index(err.argmax(), err.shape))
        raise AssertionError(f"{name}: lse of row {t} of (b={b}, h={h}) is off by {worst:.3g}x its tolerance "
                             f"({float(lse2[b, h, t]) * LN2:.9g} vs {float(ref_lse[b, h, t]):.9g})")
    return worst


def check_all(got, ref, model, q, k, scale, name="", record_as=None):
    """check() for o, dq, dk, dv and lse_check(); got: dict with o, dq, dk, dv (head-major) and lse2.
    Returns {tensor: worst ratio}. record_as = (kernel, family) also notes the ratios (see record)."""
    out = {}
    for t in ("o", "dq", "dk", "dv"):
        out[t] = check(got[t], ref[t], model[t], name=f"{name} {t}", strict=False, mag=ref.get(t + "_mag"))
    out["lse"] = lse_check(got["lse2"], ref["lse"], q, k, scale, name=f"{name} lse", strict=False)
    if record_as is not None:
        for t, r in out.items():
            record(record_as[0], record_as[1], t, r)
    for t in ("o", "dq", "dk", "dv"):  # now raise, with the tile named
        check(got[t], ref[t], model[t], name=f"{name} {t}", mag=ref.get(t + "_mag"))
    lse_check(got["lse2"], ref["lse"], q, k, scale, name=f"{name} lse")
    return out


# ------------------------------------------------------------------------------------ ratio record
_RATIOS: dict = {}
_NOTES: dict = {}


def record(kernel, family, tensor, ratio, note=False):
    """Keeps the worst ratio per (kernel, family, tensor); with ATTN_ORACLE_RATIOS=<path> in the
    environment the table is rewritten there after every update (profiles/attention_oracle_ratios.txt
    is one GPU run of tests/test_attention_oracle_gpu.py written this way)."""
    tab = _NOTES if note else _RATIOS
    key = (kernel, family, tensor)
    tab[key] = max(tab.get(key, 0.0), float(ratio))
    path = os.environ.get("ATTN_ORACLE_RATIOS")
    if not path:
        return
    lines = ["# worst kernel-to-reference error over the rounding model's, per 32-row tile (bound: "
             f"{K_BOUND:g}); lse: worst |error| / tolerance (bound: 1)",
             f"{'kernel':<28} {'family':<8} {'tensor':<4} worst"]
    lines += [f"{k_:<28} {f_:<8} {t_:<4} {r:.3f}" for (k_, f_, t_), r in sorted(_RATIOS.items())]
    if _NOTES:
        lines += ["", "# the rounding model's own worst per-tile relative error against float64"]
        lines += [f"{k_:<28} {f_:<8} {t_:<4} {r:.3e}" for (k_, f_, t_), r in sorted(_NOTES.items())]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def worst_tile_rel_error(x, ref, rows=WAVE_ROWS):
    """max over tiles of |x - ref|_F / |ref|_F of the tile (tiles below the check's floor excluded)."""
    r = ref.double()
    e, n = _tile_norms(x.double() - r, rows), _tile_norms(r, rows)
    floor = FLOOR * r.flatten(2).norm(dim=-1, keepdim=True) / math.sqrt(e.shape[-1])
    return float(torch.where(n > floor, e / n, torch.zeros_like(e)).max())
