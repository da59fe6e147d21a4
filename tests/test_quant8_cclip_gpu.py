"""The gfx950 q8 centered-clipping kernels (q8_cclip_*, csrc/kernels/compress.hip) against the torch definition
(Quant8Compressor.reduce_cclip_reference), bit for bit: the record, the weights and the non-finite counter; chunks
strided over, borders, repeatability, the optional outputs, the binding's refusals, and one simulated averaging round
end to end."""
import functools

import pytest
import torch

from distributedvolunteercomputing_amd import ops
from distributedvolunteercomputing_amd.ops import robust
from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor
from tests._q8_cclip import FAMILIES, clipping_tau, family, reference
from tests._q8_robust import BLOCK, PLANTED, codes_of, honest, scales_of, set_scales

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PS = [2, 3, 5, 8, 16]
# one q8 block, far less than a chunk | a ragged chunk | one exact chunk | a chunk plus a block | two chunks plus a block
BPS = [1, 31, 32, 33, 65]
PAD = 64  # border elements on each side: 64 B of uint8, 256 B of fp32, 512 B of int64: the inside stays 16-byte aligned
SENT = {torch.uint8: 0xA5, torch.int64: -(1 << 40), torch.float32: -7777.0}


def _bordered(n, dtype, dev):
    """(whole, inside): `inside` is n elements with PAD sentinel elements before and after it."""
    whole = torch.full((n + 2 * PAD,), SENT[dtype], dtype=dtype, device=dev)
    return whole, whole[PAD:PAD + n]


def _border_intact(whole, n):
    s = SENT[whole.dtype]
    return bool((whole[:PAD] == s).all()) and bool((whole[PAD + n:] == s).all())


def _bits(w):
    return w.view(torch.int32).tolist()


def _check_kernel(rec_cpu, mask, valid, tau, iters, gpu, tag):
    """One case: the kernels' record, weights and non-finite counter against the definition on the GPU. The input and
    every output sit in sentinel-bordered allocations, the input is only read, and a second launch gives the same
    bytes (the workspace carries no state) with the counter doubled."""
    C = ops.native()
    P, nrec = rec_cpu.shape
    m = nrec * 32 // 33
    rec = rec_cpu.to(gpu)
    want, want_w, want_bad, _ = reference(rec, mask, valid, tau, iters)
    want_bad = int(want_bad)
    recv_w, recv = _bordered(P * nrec, torch.uint8, gpu)
    recv.copy_(rec.view(-1))
    out_w, out = _bordered(nrec, torch.uint8, gpu)
    w_w, w = _bordered(P, torch.float32, gpu)
    bad_w, bad = _bordered(1, torch.int64, gpu)
    bad.zero_()
    C.q8_cclip_reduce(recv, P, m, mask, valid, tau, iters, out, w, bad)
    assert torch.equal(out, want), tag
    assert _bits(w) == _bits(want_w) and int(bad) == want_bad, (tag, w.tolist(), want_w.tolist(), int(bad), want_bad)
    assert torch.equal(recv, rec.view(-1)) and _border_intact(recv_w, P * nrec), tag  # recv is only read
    assert _border_intact(out_w, nrec) and _border_intact(w_w, P) and _border_intact(bad_w, 1), tag
    out2 = torch.empty(nrec, dtype=torch.uint8, device=gpu)
    w.fill_(SENT[torch.float32])
    C.q8_cclip_reduce(recv, P, m, mask, valid, tau, iters, out2, w, bad)
    assert torch.equal(out2, want) and _bits(w) == _bits(want_w) and int(bad) == 2 * want_bad, tag
    return want_w, want_bad


def test_definition_on_the_gpu_is_the_definition(gpu):
    """The kernel tests build their oracle with the torch definition on the GPU (the large shape would cost seconds
    on the CPU). It is the same oracle: same bytes, same weights, same counter as on the CPU, NaN, Inf and 0 * Inf
    included."""
    bps = 33
    m = bps * BLOCK
    for P in (3, 16):
        for name in FAMILIES:
            rec, mask = family(name, P, bps)
            for tau in (0.0, clipping_tau(rec, mask, m)):
                for valid in (m, m - 77):
                    oc, wc, bc, _ = reference(rec, mask, valid, tau, 3)
                    og, wg, bg, _ = reference(rec.to(gpu), mask, valid, tau, 3)
                    assert torch.equal(oc, og.cpu()) and _bits(wc) == _bits(wg.cpu()) and int(bc) == int(bg), \
                        (P, name, tau, valid)


@pytest.mark.parametrize("bps", BPS)
@pytest.mark.parametrize("P", PS)
def test_kernels_match_the_definition_bit_for_bit(gpu, P, bps):
    m = bps * BLOCK
    saw_nonfinite = 0
    saw_partial = False
    for name in FAMILIES:
        rec, mask = family(name, P, bps)
        for tau in (0.0, clipping_tau(rec.to(gpu), mask, m)):
            for iters in (1, 3):
                for valid in sorted({max(v, 0) for v in (m, m - 77, 0)}):
                    w, bad = _check_kernel(rec, mask, valid, tau, iters, gpu, (name, tau, iters, valid))
                    saw_nonfinite += bad if name == "majority_bad" else 0
                    saw_partial |= name == "far_row" and 0.0 < float(w[P - 1]) < 1.0
    assert saw_nonfinite > 0  # the frozen-coordinate path ran
    assert saw_partial or P == 2  # a weight strictly inside (0, 1): two voters are equally far from their mean


def test_garbage_row_takes_every_planted_scale(gpu):
    """bps = 1 holds one scale: the garbage row takes each planted scale in turn."""
    for seed in range(len(PLANTED)):
        rec, mask = family("garbage_row", 5, 1, seed)
        _check_kernel(rec, mask, BLOCK, 0.0, 2, gpu, ("planted", seed))


@functools.lru_cache(maxsize=None)
def _large_base(bps):
    return honest(4, bps, torch.Generator().manual_seed(7))


def test_more_chunks_than_workgroups(gpu):
    """(cap + 37) chunks plus one block: every workgroup takes a second chunk or not, and the last chunk is ragged."""
    C = ops.native()
    cap = C.q8_cclip_max_workgroups()
    assert cap == robust.CCLIP_MAX_WORKGROUPS  # the chunk is cclip's, and so is the cap
    P = 3
    bps = (cap + 37) * 32 + 1
    m = bps * BLOCK
    base = _large_base(bps)  # computed once, left unchanged
    rec = base[torch.arange(P) % 4].clone()
    sc = scales_of(rec)[1].view(torch.int32).tolist()
    for i, pattern in enumerate(PLANTED):
        sc[(i * 4099 + 5) % bps] = pattern  # a few non-finite values in row 1, spread over both trips
    sc[bps - 1] = PLANTED[0]
    set_scales(rec, 1, [x & 0xFFFFFFFF for x in sc])
    codes_of(rec)[2] = codes_of(rec)[2].flip(0)  # three different rows
    w, _ = _check_kernel(rec, 0b111, m - 77, 0.0, 2, gpu, "large")
    assert float(w[1]) == 0.0


@pytest.mark.parametrize("P", [1, 5, 16])
def test_one_voter(gpu, P):
    """The garbage row as the only voter: its non-finite decodes come out 0 and are counted."""
    for bps in (1, 33):
        m = bps * BLOCK
        rec, _ = family("garbage_row", P, bps)
        row = P // 2
        for valid in (m, m - 77 if bps > 1 else 51, 0):
            w, bad = _check_kernel(rec, 1 << row, valid, 0.0, 3, gpu, ("one voter", P, bps, valid))
            assert w.tolist() == [1.0 if k == row else 0.0 for k in range(P)]
            assert bad > 0 or valid == 0


def test_optional_outputs(gpu):
    C = ops.native()
    P, bps = 5, 33
    m = bps * BLOCK
    rec, mask = family("majority_bad", P, bps)
    want, want_w, want_bad, _ = reference(rec.to(gpu), mask, m, 0.0, 2)
    recv = rec.to(gpu).view(-1)
    for with_w in (False, True):
        for with_bad in (False, True):
            out = torch.empty(m + m // 32, dtype=torch.uint8, device=gpu)
            w = torch.zeros(P, device=gpu) if with_w else None
            bad = torch.zeros(1, dtype=torch.int64, device=gpu) if with_bad else None
            C.q8_cclip_reduce(recv, P, m, mask, m, 0.0, 2, out, w, bad)
            assert torch.equal(out, want)
            assert w is None or _bits(w) == _bits(want_w)
            assert bad is None or int(bad) == int(want_bad) > 0
    out = torch.empty(m + m // 32, dtype=torch.uint8, device=gpu)
    C.q8_cclip_reduce(recv, P, m, mask, m, 0.0, 2, out)  # both are keyword defaults
    assert torch.equal(out, want)


def test_binding_refuses_before_anything_is_written(gpu):
    C = ops.native()
    P, bps = 3, 2
    m = bps * BLOCK
    nrec = m + m // 32
    out_w, out = _bordered(nrec, torch.uint8, gpu)
    w_w, w = _bordered(16, torch.float32, gpu)
    bad_w, bad = _bordered(2, torch.int64, gpu)
    good = torch.zeros(P * nrec, dtype=torch.uint8, device=gpu)

    def call(recv=good, P=P, m=m, mask=0b111, valid=m, tau=0.0, iters=3, out_=out, weights=None, nonfinite=None):
        C.q8_cclip_reduce(recv, P, m, mask, valid, tau, iters, out_, weights, nonfinite)

    bad_calls = {
        "P = 17": lambda: call(torch.zeros(17 * nrec, dtype=torch.uint8, device=gpu), P=17, mask=(1 << 17) - 1),
        "P = 0": lambda: call(P=0, mask=1),
        "empty mask": lambda: call(mask=0),
        "mask beyond P": lambda: call(mask=0b1001),
        "m % 128": lambda: call(m=m - 8),
        "m = 0": lambda: call(m=0, valid=0),
        "valid > m": lambda: call(valid=m + 1),
        "valid < 0": lambda: call(valid=-1),
        "short recv": lambda: call(good[:-4]),
        "int8 recv": lambda: call(good.view(torch.int8)),
        "cpu recv": lambda: call(good.cpu()),
        "misaligned recv": lambda: call(torch.zeros(P * nrec + 16, dtype=torch.uint8, device=gpu)[4:4 + P * nrec]),
        "short record": lambda: call(out_=out[:nrec - 4]),
        "misaligned record": lambda: call(out_=out_w[PAD + 4:PAD + 4 + nrec]),
        "cpu record": lambda: call(out_=torch.zeros(nrec, dtype=torch.uint8)),
        "fp64 weights": lambda: call(weights=torch.zeros(P, dtype=torch.float64, device=gpu)),
        "short weights": lambda: call(weights=w[:2]),
        "long weights": lambda: call(weights=w[:4]),
        "cpu weights": lambda: call(weights=torch.zeros(P)),
        "int32 nonfinite": lambda: call(nonfinite=torch.zeros(1, dtype=torch.int32, device=gpu)),
        "long nonfinite": lambda: call(nonfinite=bad[:2]),
        "cpu nonfinite": lambda: call(nonfinite=torch.zeros(1, dtype=torch.int64)),
        "negative tau": lambda: call(tau=-1.0),
        "nan tau": lambda: call(tau=float("nan")),
        "inf tau": lambda: call(tau=float("inf")),
        "tau beyond fp32": lambda: call(tau=1e39),
        "iters = 0": lambda: call(iters=0),
        "iters = 9": lambda: call(iters=9),
    }
    for what, fn in bad_calls.items():
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            fn()
            pytest.fail(f"{what} was accepted")
    torch.cuda.synchronize()
    assert bool((out_w == SENT[torch.uint8]).all()) and bool((w_w == SENT[torch.float32]).all())
    assert bool((bad_w == SENT[torch.int64]).all())
    # the method refuses what the definition refuses, on any device
    comp = Quant8Compressor(P * m, gpu)
    ok = dict(recv=good, P=P, live_mask=0b111, valid=m, tau=0.0, iters=3)
    for kw in (dict(live_mask=0), dict(live_mask=0b1000), dict(valid=m + 1), dict(valid=-1), dict(recv=good[:-4]),
               dict(tau=-1.0), dict(tau=float("nan")), dict(tau=1e39), dict(iters=0), dict(iters=9),
               dict(weights=torch.zeros(P)), dict(nonfinite=torch.zeros(1, dtype=torch.int32, device=gpu))):
        with pytest.raises(ValueError):
            comp.reduce_cclip(**dict(ok, **kw))
    bad[:1].zero_()
    call(weights=w[:P], nonfinite=bad[:1])  # the same call with nothing wrong goes through: zeros give zeros
    assert not out.any() and w[:P].tolist() == [1.0] * P and int(bad[0]) == 0
    assert _border_intact(out_w, nrec) and bool((w_w[PAD + P:] == SENT[torch.float32]).all())


def test_averaging_round_end_to_end(gpu):
    """One simulated cclip round over q8 on the GPU (a 1-rank group exercises nothing): encode on 5 peers, one of
    which then puts NaN into its scales and one a newcomer whose all-zero records do not vote; the records shuffled
    by hand as the all-to-all leaves them; reduce_cclip on every shard owner; decode; lsgd_apply. Against the same
    calls on CPU tensors, which is the arithmetic the CPU trainer runs. Everything is bit-equal: the records by the
    kernels' contracts, and lsgd_apply with outer_lr = avg_scale = 1 multiplies by +-1 only."""
    from distributedvolunteercomputing_amd.jobs.train import nan_scales

    P, n = 5, 5 * 3 * BLOCK - 72  # a multiple of 8 (lsgd_apply's vectors) and of nothing larger: the last shard is padded
    g = torch.Generator().manual_seed(5)
    anchor = torch.randn(n, generator=g)
    deltas = (0.01 * torch.randn(P, n, generator=g)).to(BF)
    deltas[4] = 0.0  # the newcomer
    mask = robust.mask_of([0, 1, 2, 3], P)
    state = {}
    for dev in ("cpu", gpu):
        comps = [Quant8Compressor(n, dev) for _ in range(P)]
        comps[1].wire_hook = nan_scales  # the faulty peer
        L, m, rec = comps[0].layout(P)
        wires = [comps[r].encode(deltas[r].to(dev), P).view(P, rec).clone() for r in range(P)]
        weights = torch.zeros(P, P, dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        records = []
        for j in range(P):
            recv = torch.stack([wires[r][j] for r in range(P)]).reshape(-1)
            valid = min(max(n - j * m, 0), m)
            records.append(comps[j].reduce_cclip(recv, P, mask, valid, 0.0, 3, weights[j], bad).clone())
        gathered = torch.cat(records)
        avg = comps[0].decode(gathered, P)
        a = anchor.clone().to(dev)
        master = (a + 0.5).clone()
        param = torch.zeros(n, dtype=BF, device=dev)
        ops.lsgd_apply(avg, a, master, param, None, outer_lr=1.0, mu=0.0, nesterov=False, avg_scale=1.0)
        state[str(dev)] = [t.cpu() for t in (torch.stack(wires), gathered, avg.view(torch.int16), a, master,
                                              param.view(torch.int16), weights.view(torch.int32), bad,
                                              torch.stack([c.e for c in comps]))]
    for tc, tg in zip(state["cpu"], state[str(gpu)]):
        assert torch.equal(tc, tg)
    _, _, avg, a, master, _, weights, bad, _ = state[str(gpu)]
    weights = weights.view(torch.float32)
    assert torch.isfinite(avg.view(BF).float()).all() and torch.isfinite(a).all()
    assert not weights[:, 1].any() and not weights[:, 4].any() and int(bad) == 0
    assert bool((weights[:, [0, 2, 3]] > 0).all())
    assert torch.equal(a, anchor + avg.view(BF).float()) and torch.equal(master, a)
