"""The attention oracle (tests/_attn_oracle.py) checked against itself, without a GPU: it accepts the
rounding model and an independent draw of the model's rounding noise, and rejects planted bugs of
the kinds a rewritten kernel can have. Two of those bugs are local to one 32-row tile and pass the
whole-tensor `rel < 2e-2` check of tests/test_attention_gpu.py; that is asserted too, so the gap the
oracle closes stays on record."""
import math

import pytest
import torch

from tests import _attn_oracle as ao

B, H, T, D = 1, 2, 132, 64
SCALE = 1 / math.sqrt(D)
TENSORS = ("o", "dq", "dk", "dv")


def _case(family="randn", Hq=H, Hkv=H, seed=0):
    q, k, v, do = ao.make_inputs(family, B, Hq, Hkv, T, D, SCALE, seed=seed)
    return (q, k, v, do), ao.reference(q, k, v, do, SCALE)


_CACHE = {}


def _shared(key, *a, **kw):
    if key not in _CACHE:
        inp, ref = _case(*a, **kw)
        _CACHE[key] = inp, ref, ao.rounding_model(*inp, SCALE, "d64")
    return _CACHE[key]


def _verdict(got, inp, ref, model):
    """{check: worst ratio}, and whether the oracle accepts `got` (a dict like rounding_model's)."""
    q, k = inp[0], inp[1]
    w = {t: ao.check(got[t], ref[t], model[t], strict=False, mag=ref.get(t + "_mag")) for t in TENSORS}
    w["lse"] = ao.lse_check(got["lse2"], ref["lse"], q, k, SCALE, strict=False)
    ok = all(w[t] <= ao.K_BOUND for t in TENSORS) and w["lse"] <= 1.0
    return w, ok


def _old_check_passes(got, ref):
    """The whole-tensor assertions of tests/test_attention_gpu.py::test_attention_fwd_bwd."""
    ok = float((got["o"].double() - ref["o"]).abs().max()) < 2e-2
    for t in ("dq", "dk", "dv"):
        ok = ok and float((got[t].double() - ref[t]).norm() / (ref[t].norm() + 1e-6)) < 2e-2
    return ok


@pytest.mark.parametrize("kernel", ao.KERNELS)
@pytest.mark.parametrize("family", ao.FAMILIES)
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_accepts_model_and_second_draw(family, kernel, seed):
    """The model passes its own check (and lse_check, which is absolute), and so does a second,
    independent draw of its rounding noise: 32-key tiles (another stale max, so other P roundings)
    with float64 accumulation (another summation order). On two input seeds."""
    inp, ref = _case(family, seed=seed)
    model = ao.rounding_model(*inp, SCALE, kernel)
    w, ok = _verdict(model, inp, ref, model)
    assert ok, w
    second = ao.rounding_model(*inp, SCALE, kernel, key_tile=32, acc=torch.float64)
    w, ok = _verdict(second, inp, ref, model)
    print(family, kernel, seed, {t: round(r, 3) for t, r in w.items()})
    assert ok, w
    assert all(torch.isfinite(ref[t]).all() for t in ref)


def test_single_key_rows_cancel_to_zero():
    """T = 1: dq = dk = 0 exactly in the reference, so 2^-10 |ref| is 0 there; the fp32-roundoff term
    of the floor (check's `mag`) is what lets two summation orders of dP - delta pass each other,
    and it is far too small to hide a wrong value."""
    q, k, v, do = ao.make_inputs("randn", 2, 3, 3, 1, 64, SCALE, seed=1)
    ref = ao.reference(q, k, v, do, SCALE)
    assert float(ref["dq"].abs().max()) == 0 and float(ref["dk"].abs().max()) == 0
    model = ao.rounding_model(q, k, v, do, SCALE, "d64")
    second = ao.rounding_model(q, k, v, do, SCALE, "d64", key_tile=32, acc=torch.float64)
    for t in ("dq", "dk"):
        assert ao.check(second[t], ref[t], model[t], strict=False, mag=ref[t + "_mag"]) <= ao.K_BOUND
        bad = second[t] + 2.0 ** -12 * ref[t + "_mag"].float()  # 2^-12 of the cancelling terms: not roundoff
        assert ao.check(bad, ref[t], model[t], strict=False, mag=ref[t + "_mag"]) > ao.K_BOUND


def test_oracle_accepts_gqa_model():
    inp, ref = _case(Hq=4, Hkv=2)
    model = ao.rounding_model(*inp, SCALE, "hm")
    second = ao.rounding_model(*inp, SCALE, "hm", key_tile=32, acc=torch.float64)
    w, ok = _verdict(second, inp, ref, model)
    assert ok, w


def _tile_scaled(x, tile, f):
    x = x.clone()
    x[:, 1, tile * 32:(tile + 1) * 32] *= f
    return x


def _mutants():
    inp, ref, model = _shared("randn")
    q, k, v, do = inp
    out = {}
    out["mask_off_by_one"] = ao.rounding_model(*inp, SCALE, "d64", fault="mask_off_by_one")
    out["dk_tile_x1.05"] = dict(model, dk=_tile_scaled(model["dk"], 2, 1.05))
    dv = model["dv"].clone()
    dv[:, :, 128:] = 0  # the ragged last tile: rows 128..131
    out["dv_last_tile_zero"] = dict(model, dv=dv)
    out["extra_key_past_T"] = ao.rounding_model(*inp, SCALE, "d64", fault="extra_key")
    out["dq_scale_log2e"] = dict(model, dq=model["dq"] * ao.LOG2E)
    lse2 = model["lse2"].clone()
    lse2[0, 1, 77] += 2.0 ** -6 / ao.LN2  # 2^-6 in the natural log
    out["lse_row_off"] = dict(model, lse2=lse2)
    out["k_heads_swapped"] = ao.rounding_model(q, k.flip(1), v, do, SCALE, "d64")
    return out


@pytest.mark.parametrize("mutant", ["mask_off_by_one", "dk_tile_x1.05", "dv_last_tile_zero", "extra_key_past_T",
                                    "dq_scale_log2e", "lse_row_off", "k_heads_swapped"])
def test_oracle_rejects(mutant):
    inp, ref, model = _shared("randn")
    if "mutants" not in _CACHE:
        _CACHE["mutants"] = _mutants()
    w, ok = _verdict(_CACHE["mutants"][mutant], inp, ref, model)
    print(mutant, {t: round(r, 3) for t, r in w.items()})
    assert not ok, w


def test_oracle_rejects_skipped_rescale():
    """up12 rescales at every key tile; the O accumulator of key tile 1 is not multiplied by alpha."""
    inp, ref, model = _shared("up12", "up12")
    w, ok = _verdict(ao.rounding_model(*inp, SCALE, "d64", fault="skip_rescale:1"), inp, ref, model)
    assert not ok, w
    assert w["o"] > ao.K_BOUND, w


def test_oracle_rejects_gqa_wrong_group():
    """dK of each key/value head summed over the other group's query heads."""
    inp, ref = _case(Hq=4, Hkv=2)
    model = ao.rounding_model(*inp, SCALE, "hm")
    w, ok = _verdict(dict(model, dk=model["dk"].flip(1)), inp, ref, model)
    assert not ok and w["dk"] > ao.K_BOUND, w


@pytest.mark.parametrize("mutant", ["dk_tile_x1.05", "dv_last_tile_zero"])
def test_whole_tensor_check_misses_tile_local_bugs(mutant):
    """The gap: one wrong 32-row tile passes test_attention_fwd_bwd's whole-tensor assertions."""
    inp, ref, model = _shared("randn")
    if "mutants" not in _CACHE:
        _CACHE["mutants"] = _mutants()
    assert _old_check_passes(model, ref)
    assert _old_check_passes(_CACHE["mutants"][mutant], ref)
    assert not _verdict(_CACHE["mutants"][mutant], inp, ref, model)[1]


def test_check_rejects_nan_and_reports_tile():
    inp, ref, model = _shared("randn")
    bad = model["dq"].clone()
    bad[0, 1, 40, 3] = float("nan")
    assert ao.check(bad, ref["dq"], model["dq"], strict=False) == float("inf")
    with pytest.raises(AssertionError, match=r"rows 32\.\.63 of \(b=0, h=1\)"):
        ao.check(bad, ref["dq"], model["dq"], name="dq")


def test_packed_adapter_round_trip():
    q, k, v, do = ao.make_inputs("randn", 2, 3, 3, 5, 64, SCALE)
    qkv = ao.pack_qkv(q, k, v)
    assert qkv.shape == (2, 5, 3, 3, 64) and qkv.is_contiguous()
    for a, b in zip(ao.unpack_dqkv(qkv), (q, k, v)):
        assert torch.equal(a, b)
    ref = ao.reference_packed(qkv, ao.token_major(do), SCALE)
    assert torch.equal(ref["dq"], ao.reference(q, k, v, do, SCALE)["dq"])


def test_prescale_rounding_cost_is_visible_on_wide3():
    """The d64 dQ kernels' bf16(Q * c) costs accuracy where scores are large: the model with that
    rounding is further from float64 than without it on wide3 (figures in
    profiles/attention_oracle_ratios.txt)."""
    inp, ref = _case("wide3")
    e = {p: ao.worst_tile_rel_error(ao.rounding_model(*inp, SCALE, "d64", prescale=p)["dq"], ref["dq"])
         for p in (True, False)}
    print(e)
    assert e[True] > e[False]
