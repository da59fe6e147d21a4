"""The gfx950 q8 trimmed-mean kernel (q8_trimmed_reduce_kernel, csrc/kernels/compress.hip) against the torch
definition (Quant8Compressor.reduce_robust_reference), bit for bit: the record, the counts and the non-finite
counter, the grid-stride loop, borders, repeatability, the bindings' refusals, and one simulated averaging
round end to end."""
import functools

import pytest
import torch

from distributedvolunteercomputing_amd import ops
from distributedvolunteercomputing_amd.ops import robust
from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor
from tests._q8_robust import BLOCK, FAMILIES, PLANTED, codes_of, family, honest, scales_of, set_scales

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PS = [2, 3, 5, 8, 16]
BPS = [1, 33]  # rec = 132: records 4-byte aligned only | a ragged last workgroup (528 units: 2 full blocks + 16 lanes)
PAD = 64  # border elements on each side: 64 B of uint8, 512 B of int64, so the inside stays 16-byte aligned
SENT_U8, SENT_I64 = 0xA5, -(1 << 40)


def _bordered(n, dtype, dev):
    """(whole, inside): `inside` is n elements with PAD sentinel elements before and after it."""
    whole = torch.full((n + 2 * PAD,), SENT_I64 if dtype == torch.int64 else SENT_U8, dtype=dtype, device=dev)
    return whole, whole[PAD:PAD + n]


def _border_intact(whole, n):
    s = SENT_I64 if whole.dtype == torch.int64 else SENT_U8
    return bool((whole[:PAD] == s).all()) and bool((whole[PAD + n:] == s).all())


def _trims(K):
    return sorted({0, 1, (K - 1) // 2})  # plain mean, one at each end, median


def _oracle(rec, trim, mask, valid):
    """(record, counts list, nonfinite) of the torch definition on rec's device."""
    P = rec.shape[0]
    _, f, _ = robust.trim_plan(P, trim, mask)
    out, c, bad = Quant8Compressor.reduce_robust_reference(rec.reshape(-1), P, f, mask, valid)
    return out, c.tolist(), int(bad)


def _check_kernel(rec_cpu, mask, trim, valid, gpu, tag):
    """One case: the kernel's record, counts and non-finite counter against the definition on the GPU; outputs in
    sentinel-bordered allocations, the input only read, a second launch the same bytes with the counters doubled."""
    C = ops.native()
    P, nrec = rec_cpu.shape
    m = nrec * 32 // 33
    rec = rec_cpu.to(gpu)
    want, want_counts, want_bad = _oracle(rec, trim, mask, valid)
    recv = rec.clone().view(-1)
    out_w, out = _bordered(nrec, torch.uint8, gpu)
    cnt_w, cnt = _bordered(P, torch.int64, gpu)
    bad_w, bad = _bordered(1, torch.int64, gpu)
    cnt.zero_()
    bad.zero_()
    C.q8_trimmed_reduce(recv, P, m, trim, mask, valid, out, cnt, bad)
    assert torch.equal(out, want), tag
    assert cnt.tolist() == want_counts and int(bad) == want_bad, (tag, cnt.tolist(), want_counts, int(bad), want_bad)
    assert torch.equal(recv, rec.view(-1)), tag  # recv is only read
    assert _border_intact(out_w, nrec) and _border_intact(cnt_w, P) and _border_intact(bad_w, 1), tag
    out2 = torch.empty(nrec, dtype=torch.uint8, device=gpu)
    C.q8_trimmed_reduce(recv, P, m, trim, mask, valid, out2, cnt, bad)
    assert torch.equal(out2, want), tag
    assert cnt.tolist() == [2 * c for c in want_counts] and int(bad) == 2 * want_bad, tag
    out3 = torch.empty(nrec, dtype=torch.uint8, device=gpu)
    C.q8_trimmed_reduce(recv, P, m, trim, mask, valid, out3)  # both counters are optional
    assert torch.equal(out3, want), tag
    return want_bad


def test_definition_on_the_gpu_is_the_definition(gpu):
    """The kernel tests build their oracle with the torch definition on the GPU (the large shape would cost seconds
    on the CPU). It is the same oracle: same bytes, same counters as on the CPU, subnormal scales, NaN, Inf and
    0 * Inf included."""
    for P in (3, 16):
        for name in FAMILIES:
            for trim in _trims(P):
                rec, mask = family(name, P, 33, f=trim)
                m = 33 * BLOCK
                for valid in (m, m - 5):
                    oc, cc, bc = _oracle(rec, trim, mask, valid)
                    og, cg, bg = _oracle(rec.to(gpu), trim, mask, valid)
                    assert torch.equal(oc, og.cpu()) and cc == cg and bc == bg, (P, name, trim, valid)


@pytest.mark.parametrize("bps", BPS)
@pytest.mark.parametrize("P", PS)
def test_kernel_matches_the_definition_bit_for_bit(gpu, P, bps):
    m = bps * BLOCK
    saw_nonfinite = 0
    for name in FAMILIES:
        K = bin(family(name, P, bps)[1]).count("1")
        for trim in _trims(K):
            # bps = 1 holds one scale: the garbage row takes each planted scale in turn
            seeds = range(len(PLANTED)) if (name == "garbage_row" and bps == 1) else (0,)
            for seed in seeds:
                rec, mask = family(name, P, bps, seed, f=trim)
                for valid in sorted({v for v in (m, m - 5, 131, 0) if v <= m}):
                    if seed and valid != m:
                        continue
                    bad = _check_kernel(rec, mask, trim, valid, gpu, (name, trim, seed, valid))
                    saw_nonfinite += bad if name == "over_budget" else 0
    assert saw_nonfinite > 0  # the non-finite path ran


@functools.lru_cache(maxsize=None)
def _large_base(bps):
    return honest(4, bps, torch.Generator().manual_seed(7))


@pytest.mark.parametrize("P", [3, 16])
def test_grid_stride_loop(gpu, P):
    """The smallest shard that takes a second trip through the launcher's grid: one block more than max_blocks
    workgroups of 256 lanes x 8 elements cover."""
    bps = ops.native().q8_trimmed_reduce_max_blocks() * 256 // 16 + 1
    m = bps * BLOCK
    base = _large_base(bps)  # computed once, shared, left unchanged: rows repeat, which adds ties
    rec = base[torch.arange(P) % 4].clone()
    g = torch.Generator().manual_seed(P)
    bad = P // 2
    rec[bad] = torch.randint(0, 256, (rec.shape[1],), generator=g, dtype=torch.uint8)
    codes_of(rec)[bad, ::7] = -128
    sc = scales_of(rec)[bad].view(torch.int32).tolist()
    for i, pattern in enumerate(PLANTED):
        sc[(i * 4099 + 5) % bps] = pattern  # spread over both trips
    sc[bps - 1] = PLANTED[0]
    set_scales(rec, bad, [x & 0xFFFFFFFF for x in sc])
    _check_kernel(rec, (1 << P) - 1, 1, m - 5, gpu, ("large", P))


@pytest.mark.parametrize("P", PS)
def test_trim_zero_is_the_q8_reduce_kernel(gpu, P):
    bps = 33
    m = bps * BLOCK
    rec, mask = family("honest", P, bps)
    comp = Quant8Compressor(P * m, gpu)
    recv = rec.to(gpu).view(-1)
    want = comp.reduce(recv, P).clone()
    counts = torch.zeros(P, dtype=torch.int64, device=gpu)
    bad = torch.zeros(1, dtype=torch.int64, device=gpu)
    got = comp.reduce_robust(recv, P, 0, mask, m, counts, bad)
    assert torch.equal(got, want) and counts.tolist() == [0] * P and int(bad) == 0


def test_bindings_refuse_before_anything_is_written(gpu):
    C = ops.native()
    P, bps = 3, 2
    m = bps * BLOCK
    nrec = m + m // 32
    out_w, out = _bordered(nrec, torch.uint8, gpu)
    cnt_w, cnt = _bordered(16, torch.int64, gpu)
    good = torch.zeros(P * nrec, dtype=torch.uint8, device=gpu)

    def call(recv=good, P=P, m=m, trim=1, mask=0b111, valid=m, out_=out, counts=None, nonfinite=None):
        C.q8_trimmed_reduce(recv, P, m, trim, mask, valid, out_, counts, nonfinite)

    bad_calls = {
        "P = 17": lambda: call(torch.zeros(17 * nrec, dtype=torch.uint8, device=gpu), P=17, mask=(1 << 17) - 1),
        "P = 0": lambda: call(P=0, mask=1),
        "empty mask": lambda: call(mask=0),
        "mask beyond P": lambda: call(mask=0b1001),
        "m % 128": lambda: call(m=m - 8),
        "m = 0": lambda: call(m=0, valid=0),
        "short recv": lambda: call(good[:-4]),
        "int8 recv": lambda: call(good.view(torch.int8)),
        "cpu recv": lambda: call(good.cpu()),
        "misaligned recv": lambda: call(torch.zeros(P * nrec + 16, dtype=torch.uint8, device=gpu)[4:4 + P * nrec]),
        "short record": lambda: call(out_=out[:nrec - 4]),
        "misaligned record": lambda: call(out_=out_w[PAD + 4:PAD + 4 + nrec]),
        "cpu record": lambda: call(out_=torch.zeros(nrec, dtype=torch.uint8)),
        "valid < 0": lambda: call(valid=-1),
        "valid > m": lambda: call(valid=m + 1),
        "negative trim": lambda: call(trim=-1),
        "int32 counts": lambda: call(counts=torch.zeros(P, dtype=torch.int32, device=gpu)),
        "short counts": lambda: call(counts=cnt[:2]),
        "cpu counts": lambda: call(counts=torch.zeros(P, dtype=torch.int64)),
        "long nonfinite": lambda: call(nonfinite=cnt[:2]),
        "int32 nonfinite": lambda: call(nonfinite=torch.zeros(1, dtype=torch.int32, device=gpu)),
    }
    for what, fn in bad_calls.items():
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            fn()
            pytest.fail(f"{what} was accepted")
    torch.cuda.synchronize()
    assert bool((out_w == SENT_U8).all()) and bool((cnt_w == SENT_I64).all())
    # the method refuses what the definition refuses, on any device
    comp = Quant8Compressor(P * m, gpu)
    for kw in (dict(live_mask=0), dict(live_mask=0b1000), dict(valid=m + 1), dict(valid=-1), dict(recv=good[:-4])):
        args = dict(recv=good, P=P, trim=1, live_mask=0b111, valid=m)
        args.update(kw)
        with pytest.raises(ValueError):
            comp.reduce_robust(**args)
    call()  # and the same call with nothing wrong goes through: all-zero records give an all-zero record
    assert not out.any() and _border_intact(out_w, nrec) and bool((cnt_w == SENT_I64).all())


def test_averaging_round_end_to_end(gpu):
    """One simulated robust round over q8 on the GPU (a 1-rank group exercises nothing): encode on 5 peers, one of
    which then puts NaN into its scales and one a newcomer whose all-zero records do not vote; the records shuffled
    by hand as the all-to-all leaves them; reduce_robust on every shard owner; decode; lsgd_apply. Against the same
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
        counts = torch.zeros(P, dtype=torch.int64, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        records = []
        for j in range(P):
            recv = torch.stack([wires[r][j] for r in range(P)]).reshape(-1)
            valid = min(max(n - j * m, 0), m)
            records.append(comps[j].reduce_robust(recv, P, 1, mask, valid, counts, bad).clone())
        gathered = torch.cat(records)
        avg = comps[0].decode(gathered, P)
        a = anchor.clone().to(dev)
        master = (a + 0.5).clone()
        param = torch.zeros(n, dtype=BF, device=dev)
        ops.lsgd_apply(avg, a, master, param, None, outer_lr=1.0, mu=0.0, nesterov=False, avg_scale=1.0)
        state[str(dev)] = [t.cpu() for t in (torch.stack(wires), gathered, avg.view(torch.int16), a, master,
                                              param.view(torch.int16), counts, bad, torch.stack([c.e for c in comps]))]
    for tc, tg in zip(state["cpu"], state[str(gpu)]):
        assert torch.equal(tc, tg)
    _, _, avg, a, master, _, counts, bad, _ = state[str(gpu)]
    assert torch.isfinite(avg.view(BF).float()).all() and torch.isfinite(a).all()
    assert int(counts[1]) == n and int(counts[4]) == 0 and int(bad) == 0 and int(counts.sum()) == 2 * n
    assert torch.equal(a, anchor + avg.view(BF).float()) and torch.equal(master, a)
