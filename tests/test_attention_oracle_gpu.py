"""The HIP attention kernels against the per-tile float64 oracle of tests/_attn_oracle.py: every
32-row tile of o, dq, dk, dv within K = 4 times the error of an fp32 model that rounds where the
kernel rounds, and lse within an fp32-roundoff tolerance per row. Tile-edge lengths (both dK/dV
kernels, the ring's steady-state loop with ragged tails), softmax stress (stale max, a rescale at
every tile, underflowing tiles, wide scores, other scales), isolation of one (batch, head) from NaN
neighbours, every launch variant, and the head-major GQA kernels. K and the floor are not tuned to
pass (see the helper); profiles/attention_oracle_ratios.txt holds one run's worst ratios."""
import math

import pytest
import torch

from distributedvolunteercomputing_amd import ops
from tests import _attn_oracle as ao

pytestmark = pytest.mark.gpu

SCALE64 = 1 / math.sqrt(64)
DEFAULT_VARIANT = (3, 2, 12, 1)  # csrc/kernels/attention.hip g_fwd_wpe, g_fwd_dma, g_bwd_dma, g_stage_epi
VARIANTS = [(2, 0, 0, 0), (3, 0, 3, 1), (2, 1, 2, 1), (3, 1, 1, 0), (3, 1, 1, 1), (2, 2, 4, 1), (3, 2, 8, 1),
            DEFAULT_VARIANT]  # the list of tests/test_attention_gpu.py::test_attention_deterministic
EDGE_T = [1, 3, 4, 31, 32, 33, 60, 63, 64, 65, 68, 127, 128, 129, 132, 191, 193, 255, 257, 320, 321, 448, 452]


# ------------------------------------------------------------------------------------ runners
def _run_d64(q, k, v, do, scale):
    """attention.hip through the raw bindings; head-major results like the oracle's."""
    C = ops.native()
    qkv, do_tm = ao.pack_qkv(q, k, v), ao.token_major(do)
    out, lse2 = C.attn_fwd(qkv, scale)
    dq, dk, dv = ao.unpack_dqkv(C.attn_bwd(qkv, out, do_tm, lse2, scale))
    return {"o": out.transpose(1, 2), "lse2": lse2, "dq": dq, "dk": dk, "dv": dv}


def _run_hm(q, k, v, do, scale):
    """attention_hm.hip: q [B, Hq, T, D], k / v [B, Hkv, T, D]; o and do token-major."""
    C = ops.native()
    out, lse2 = C.attn_hm_fwd(q, k, v, scale)
    dq, dk, dv = C.attn_hm_bwd(q, k, v, out, ao.token_major(do), lse2, scale)
    return {"o": out.transpose(1, 2), "lse2": lse2, "dq": dq, "dk": dk, "dv": dv}


_RUN = {"d64": _run_d64, "hm": _run_hm}
_ORACLE = {}  # (kernel model, family, shape, scale, seed) -> inputs, reference, model: computed once, never modified


def _oracle(kernel, family, B, Hq, Hkv, T, D, scale, seed, dev):
    key = (kernel, family, B, Hq, Hkv, T, D, scale, seed)
    if key not in _ORACLE:
        inp = ao.make_inputs(family, B, Hq, Hkv, T, D, scale, seed=seed, device=dev)
        _ORACLE[key] = inp, ao.reference(*inp, scale), ao.rounding_model(*inp, scale, kernel)
    return _ORACLE[key]


def _case(dev, kernel, family, B, Hq, Hkv, T, D, scale, label, seed=None):
    inp, ref, model = _oracle(kernel, family, B, Hq, Hkv, T, D, scale, T if seed is None else seed, dev)
    got = _RUN[kernel](*inp, scale)
    name = f"{label} {family} B={B} Hq={Hq} Hkv={Hkv} T={T} D={D} scale={scale:.4g}"
    w = ao.check_all(got, ref, model, inp[0], inp[1], scale, name=name, record_as=(label, family))
    print(name, {t: round(r, 3) for t, r in w.items()})
    return got


# ------------------------------------------------------------------------------------ d64: tile edges, stress
@pytest.mark.parametrize("family", ["randn", "wide3"])
@pytest.mark.parametrize("T", EDGE_T)
def test_d64_tile_edges(gpu, T, family):
    """Both parities of T % 4 (ring and two-buffer dK/dV kernels), one row into a new 32 / 64 / 128
    block, single-tile lengths, and the ring's 3-slot steady-state loop (T >= 320) with ragged tails."""
    _case(gpu, "d64", family, 2, 3, 3, T, 64, SCALE64, "d64 default")


@pytest.mark.parametrize("T", [200, 452])
@pytest.mark.parametrize("family", ["up5", "up12", "down12", "wide3"])
def test_d64_softmax_stress(gpu, family, T):
    """Stale-max tiles alternating with rescales (up5), a rescale at every key tile (up12), the max in
    the first tile and later tiles underflowing (down12), wide scores (wide3)."""
    _case(gpu, "d64", family, 2, 3, 3, T, 64, SCALE64, "d64 default", seed=1000 + T)


@pytest.mark.parametrize("scale", [0.03, 0.125, 0.5])
def test_d64_scale(gpu, scale):
    _case(gpu, "d64", "randn", 2, 3, 3, 200, 64, scale, "d64 default", seed=7)


def test_d64_prescale_cost_on_record(gpu):
    """The accuracy cost of folding the score scale into bf16 Q in the dQ kernels (attn_common.h
    prescale): the model's own dQ error against float64 with and without that rounding, on wide3."""
    inp, ref, model = _oracle("d64", "wide3", 2, 3, 3, 452, 64, SCALE64, 1452, gpu)
    with_p = ao.worst_tile_rel_error(model["dq"], ref["dq"])
    without = ao.worst_tile_rel_error(ao.rounding_model(*inp, SCALE64, "d64", prescale=False)["dq"], ref["dq"])
    ao.record("model d64, prescale", "wide3", "dq", with_p, note=True)
    ao.record("model d64, no prescale", "wide3", "dq", without, note=True)
    assert math.isfinite(with_p) and math.isfinite(without)
    assert with_p > without  # the rounding is real: dropping it from the model would loosen nothing unnoticed


# ------------------------------------------------------------------------------------ d64: isolation
def _isolated_inputs(dev, T, keep, seed):
    """randn B = 3, H = 3 inputs and a copy with NaN in every (batch, head) slot that `keep` (a bool
    [B, H] mask) does not select, in q, k, v and dO alike."""
    inp = ao.make_inputs("randn", 3, 3, 3, T, 64, SCALE64, seed=seed, device=dev)
    hole = ~keep.to(dev)[:, :, None, None]
    return inp, tuple(t.masked_fill(hole, float("nan")) for t in inp)


@pytest.mark.parametrize("T", [77, 200])
def test_d64_isolation(gpu, T):
    """One (batch, head) computes the same bits whether its neighbours hold numbers or NaN (the
    clamped row reads and the buffer-resource bounds keep a block inside its own rows), and passes
    the oracle."""
    b, h = 1, 1
    keep = torch.zeros(3, 3, dtype=torch.bool)
    keep[b, h] = True
    clean, holed = _isolated_inputs(gpu, T, keep, seed=40 + T)
    ga, gb = _run_d64(*clean, SCALE64), _run_d64(*holed, SCALE64)
    for t in ("o", "lse2", "dq", "dk", "dv"):
        x, y = ga[t][b, h], gb[t][b, h]
        assert torch.isfinite(y.float()).all(), t
        assert torch.equal(x, y), f"{t} of (b={b}, h={h}) depends on its neighbours"
    one = tuple(t[b:b + 1, h:h + 1] for t in clean)
    ref, model = ao.reference(*one, SCALE64), ao.rounding_model(*one, SCALE64, "d64")
    got = {t: gb[t][b:b + 1, h:h + 1] for t in gb}
    ao.check_all(got, ref, model, one[0], one[1], SCALE64, name=f"d64 isolated T={T}", record_as=("d64 isolated", "randn"))


@pytest.mark.parametrize("T", [77, 200])
def test_d64_isolation_bias_grad(gpu, T):
    """The fused QKV-bias gradient of one head: its 3 x 64 columns sum that head's dq / dk / dv rows
    over every batch, so here the whole head (all batches) keeps its numbers and every OTHER head
    holds NaN. The columns must be finite and the same bits as with numbers everywhere."""
    C = ops.native()
    h, H = 1, 3
    keep = torch.zeros(3, 3, dtype=torch.bool)
    keep[:, h] = True
    clean, holed = _isolated_inputs(gpu, T, keep, seed=60 + T)
    db = []
    for q, k, v, do in (clean, holed):
        qkv, do_tm = ao.pack_qkv(q, k, v), ao.token_major(do)
        out, lse2 = C.attn_fwd(qkv, SCALE64)
        dqkv, g = C.attn_bwd_bias(qkv, out, do_tm, lse2, SCALE64, None)
        db.append((g.view(3, H, 64)[:, h], dqkv[:, :, :, h]))
    (ga, da), (gb, dg) = db
    assert torch.isfinite(gb.float()).all()
    assert torch.equal(ga, gb), "bias-gradient columns of one head depend on the other heads"
    assert torch.equal(da, dg)
    # and they are that head's column sums (the tolerance of test_attention_fused_qkv_bias_grad)
    ref = dg.float().sum((0, 1))
    assert float((gb.float() - ref).norm() / ref.norm()) < 1e-2


# ------------------------------------------------------------------------------------ d64: variants
@pytest.mark.parametrize("T", [77, 132, 452])
@pytest.mark.parametrize("variant", VARIANTS)
def test_d64_variants(gpu, variant, T):
    """Every launch variant is right, not only repeatable."""
    C = ops.native()
    C.attn_set_variant(*variant)
    try:
        _case(gpu, "d64", "wide3" if T == 452 else "randn", 2, 3, 3, T, 64, SCALE64,
              "d64 variant " + ",".join(map(str, variant)), seed=2000 + T)
    finally:
        C.attn_set_variant(*DEFAULT_VARIANT)


@pytest.mark.parametrize("family", ["randn", "wide3"])
@pytest.mark.parametrize("T", [200, 452])
def test_d64_ring_kernels_bit_identical_to_two_buffer(gpu, T, family):
    """What the comments at attention.hip's defaults promise: the 3-slot ring kernels compute the
    same bits as the two-buffer LDS-DMA kernels (forward fwd_dma 2 vs 1; backward bwd_dma 12 vs 3)."""
    C = ops.native()
    q, k, v, do = ao.make_inputs(family, 2, 3, 3, T, 64, SCALE64, seed=3000 + T, device=gpu)
    qkv, do_tm = ao.pack_qkv(q, k, v), ao.token_major(do)
    try:
        C.attn_set_variant(3, 1, 3, 1)
        o1, l1 = C.attn_fwd(qkv, SCALE64)
        C.attn_set_variant(3, 2, 3, 1)
        o2, l2 = C.attn_fwd(qkv, SCALE64)
        assert torch.equal(o1, o2) and torch.equal(l1, l2), "forward: ring vs two-buffer"
        g3 = C.attn_bwd(qkv, o1, do_tm, l1, SCALE64)
        C.attn_set_variant(3, 2, 12, 1)
        g12 = C.attn_bwd(qkv, o1, do_tm, l1, SCALE64)
        for i, nm in enumerate(("dq", "dk", "dv")):
            assert torch.equal(g3[:, :, i], g12[:, :, i]), f"backward {nm}: ring vs two-buffer"
    finally:
        C.attn_set_variant(*DEFAULT_VARIANT)


# ------------------------------------------------------------------------------------ GQA (attention_hm.hip)
GQA_T = [1, 63, 64, 65, 129, 200, 452]
GQA_HEADS = [(4, 2), (6, 1), (2, 2)]


@pytest.mark.parametrize("family", ["randn", "wide3", "up12", "down12"])
@pytest.mark.parametrize("T", GQA_T)
@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_gqa(gpu, D, Hq, Hkv, T, family):
    _case(gpu, "hm", family, 2, Hq, Hkv, T, D, 1 / math.sqrt(D), f"hm d{D}")


@pytest.mark.parametrize("family", ["randn", "wide3", "up12", "down12"])
@pytest.mark.parametrize("T", GQA_T)
@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
def test_gqa_d128_split_dkdv(gpu, Hq, Hkv, T, family):
    """D = 128 with dK and dV as two launches (the non-default variant), same oracle."""
    C = ops.native()
    C.attn_hm_set_variant(1)
    try:
        _case(gpu, "hm", family, 2, Hq, Hkv, T, 128, 1 / math.sqrt(128), "hm d128 split")
    finally:
        C.attn_hm_set_variant(0)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [77, 200])
def test_gqa_isolation(gpu, T, D):
    """One key/value group (kv head 1 of batch 1 with its query heads 2, 3) against NaN in every
    other group and batch: same bits, finite, and right."""
    b, hk, Hq, Hkv = 1, 1, 4, 2
    rep = Hq // Hkv
    scale = 1 / math.sqrt(D)
    clean = ao.make_inputs("randn", 2, Hq, Hkv, T, D, scale, seed=80 + T, device=gpu)
    keepq = torch.zeros(2, Hq, dtype=torch.bool, device=gpu)
    keepq[b, hk * rep:(hk + 1) * rep] = True
    keepk = torch.zeros(2, Hkv, dtype=torch.bool, device=gpu)
    keepk[b, hk] = True
    holed = tuple(t.masked_fill(~(keepq if t.shape[1] == Hq else keepk)[:, :, None, None], float("nan"))
                  for t in clean)
    ga, gb = _run_hm(*clean, scale), _run_hm(*holed, scale)

    def mine(t, x):
        hs = slice(hk, hk + 1) if t in ("dk", "dv") else slice(hk * rep, (hk + 1) * rep)
        return x[b:b + 1, hs]

    for t in ("o", "lse2", "dq", "dk", "dv"):
        x, y = mine(t, ga[t]), mine(t, gb[t])
        assert torch.isfinite(y.float()).all(), t
        assert torch.equal(x, y), f"{t} of kv group (b={b}, hk={hk}) depends on its neighbours"
    one = (clean[0][b:b + 1, hk * rep:(hk + 1) * rep], clean[1][b:b + 1, hk:hk + 1], clean[2][b:b + 1, hk:hk + 1],
           clean[3][b:b + 1, hk * rep:(hk + 1) * rep])
    ref, model = ao.reference(*one, scale), ao.rounding_model(*one, scale, "hm")
    got = {t: mine(t, gb[t]) for t in gb}
    ao.check_all(got, ref, model, one[0], one[1], scale, name=f"hm isolated T={T} D={D}",
                 record_as=(f"hm d{D} isolated", "randn"))
