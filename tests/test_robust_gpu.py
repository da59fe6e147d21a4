"""The gfx950 trimmed-mean kernel (csrc/kernels/robust.hip) against the torch definition
(ops/robust.py), bit for bit: results, counts, aliasing, borders, repeatability, the bindings'
refusals, and the averaging round's arithmetic end to end."""
import pytest
import torch

from distributedvolunteercomputing_amd import ops
from distributedvolunteercomputing_amd.ops import robust
from tests._robust import FAMILIES, bits, family

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PS = [2, 3, 5, 8, 16]
NS = [8, 4104, 31 * 1024 * 8]  # one vector, a ragged last block, the grid-stride loop
PAD = 64  # border elements on each side: 128 B of bf16, 512 B of int64, so the inside stays 16-byte aligned
SENT_BF, SENT_I64 = -7.0, -(1 << 40)


def _bordered(n, dtype, dev):
    """(whole, inside): `inside` is n elements with PAD sentinel elements before and after it."""
    whole = torch.full((n + 2 * PAD,), SENT_I64 if dtype == torch.int64 else SENT_BF, dtype=dtype, device=dev)
    return whole, whole[PAD:PAD + n]


def _border_intact(whole, n):
    s = SENT_I64 if whole.dtype == torch.int64 else SENT_BF
    return bool((whole[:PAD] == s).all()) and bool((whole[PAD + n:] == s).all())


def _trims(K):
    return sorted({0, 1, (K - 1) // 2})  # plain mean, one at each end, median


def test_reference_on_the_gpu_is_the_reference(gpu):
    """The kernel tests build their oracle with the torch definition on the GPU (the large shapes would
    cost seconds on the CPU). It is the same oracle: same bits, same counts as on the CPU."""
    for P in (3, 16):
        for name in FAMILIES:
            x, mask = family(name, P, 4104)
            for trim in _trims(bin(mask).count("1")):
                rc, cc = ops.trimmed_mean_reference(x, trim, mask)
                rg, cg = ops.trimmed_mean_reference(x.to(gpu), trim, mask)
                assert torch.equal(bits(rc), bits(rg).cpu()) and cc.tolist() == cg.tolist(), (P, name, trim)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("P", PS)
def test_kernel_matches_the_definition_bit_for_bit(gpu, P, n):
    for name in FAMILIES:
        xc, mask = family(name, P, n)
        x = xc.to(gpu)
        for trim in _trims(bin(mask).count("1")):
            tag = (name, trim)
            ref, ref_counts = ops.trimmed_mean_reference(x, trim, mask)
            inp = x.clone().view(-1)
            mine_w, mine = _bordered(n, BF, gpu)
            out_w, out = _bordered(P * n, BF, gpu)
            cnt_w, cnt = _bordered(P, torch.int64, gpu)
            cnt.zero_()
            ops.trimmed_reduce_bcast_bf16(inp, out, mine, P, trim, mask, cnt)
            assert torch.equal(bits(mine), bits(ref)), tag
            assert torch.equal(bits(out).view(P, n), bits(ref).unsqueeze(0).expand(P, n)), tag
            assert cnt.tolist() == ref_counts.tolist(), tag
            assert torch.equal(inp.view(torch.int16), x.view(-1).view(torch.int16)), tag  # the input is only read
            assert _border_intact(mine_w, n) and _border_intact(out_w, P * n) and _border_intact(cnt_w, P), tag
            # a second launch on the same input: same bits, same counts (they add up)
            mine2 = torch.empty(n, dtype=BF, device=gpu)
            ops.trimmed_reduce_bcast_bf16(inp, out, mine2, P, trim, mask, cnt)
            assert torch.equal(bits(mine2), bits(mine)), tag
            assert cnt.tolist() == (2 * ref_counts).tolist(), tag
            # out aliasing in, as in the collective: the same bits in every row
            mine3 = torch.empty(n, dtype=BF, device=gpu)
            ops.trimmed_reduce_bcast_bf16(inp, inp, mine3, P, trim, mask, None)
            assert torch.equal(bits(mine3), bits(ref)), tag
            assert torch.equal(bits(inp).view(P, n), bits(ref).unsqueeze(0).expand(P, n)), tag


def test_outputs_are_optional(gpu):
    P, n = 5, 4104
    x, mask = family("bad_row", P, n)
    x = x.to(gpu)
    ref, ref_counts = ops.trimmed_mean_reference(x, 1, mask)
    cnt = torch.zeros(P, dtype=torch.int64, device=gpu)
    ops.trimmed_reduce_bcast_bf16(x.view(-1), None, None, P, 1, mask, cnt)
    assert cnt.tolist() == ref_counts.tolist() and int(cnt[P // 2]) == n
    out = torch.empty(P * n, dtype=BF, device=gpu)
    ops.trimmed_reduce_bcast_bf16(x.view(-1), out, None, P, 1, mask, None)
    assert torch.equal(bits(out).view(P, n)[P - 1], bits(ref)) and torch.isfinite(out.float()).all()


def test_bindings_refuse_before_anything_is_written(gpu):
    C = ops.native()
    n = 64
    mine_w, mine = _bordered(n, BF, gpu)
    cnt_w, cnt = _bordered(16, torch.int64, gpu)

    def call(inp, P, mask, out=None, mine_=mine, counts=None, trim=1):
        C.trimmed_reduce_bcast_bf16(inp, out, mine_, P, trim, mask, 1.0, counts)

    good = torch.zeros(3 * n, dtype=BF, device=gpu)
    bad_calls = {
        "P = 17": lambda: call(torch.zeros(17 * n, dtype=BF, device=gpu), 17, (1 << 17) - 1),
        "P = 0": lambda: call(good, 0, 1),
        "empty mask": lambda: call(good, 3, 0),
        "mask beyond P": lambda: call(good, 3, 0b1001),
        "n % 8": lambda: call(torch.zeros(3 * 12, dtype=BF, device=gpu), 3, 0b111, mine_=mine[:12]),
        "numel % P": lambda: call(torch.zeros(3 * n + 8, dtype=BF, device=gpu), 3, 0b111),
        "fp32 in": lambda: call(torch.zeros(3 * n, device=gpu), 3, 0b111),
        "fp32 mine": lambda: call(good, 3, 0b111, mine_=torch.zeros(n, device=gpu)),
        "cpu in": lambda: call(torch.zeros(3 * n, dtype=BF), 3, 0b111),
        "misaligned in": lambda: call(torch.zeros(3 * n + 8, dtype=BF, device=gpu)[4:4 + 3 * n], 3, 0b111),
        "misaligned mine": lambda: call(good, 3, 0b111, mine_=mine_w[PAD + 4:PAD + 4 + n]),
        "short mine": lambda: call(good, 3, 0b111, mine_=mine[:n - 8]),
        "short out": lambda: call(good, 3, 0b111, out=torch.zeros(2 * n, dtype=BF, device=gpu)),
        "int32 counts": lambda: call(good, 3, 0b111, counts=torch.zeros(3, dtype=torch.int32, device=gpu)),
        "short counts": lambda: call(good, 3, 0b111, counts=cnt[:2]),
        "negative trim": lambda: call(good, 3, 0b111, trim=-1),
    }
    for what, fn in bad_calls.items():
        with pytest.raises((RuntimeError, ValueError)):
            fn()
            pytest.fail(f"{what} was accepted")
    torch.cuda.synchronize()
    assert bool((mine_w == SENT_BF).all()) and bool((cnt_w == SENT_I64).all())
    # the op refuses what the reference refuses, on any device
    with pytest.raises(ValueError):
        ops.trimmed_reduce_bcast_bf16(torch.zeros(17 * n, dtype=BF, device=gpu), None, mine, 17, 1)
    with pytest.raises(ValueError):
        ops.trimmed_reduce_bcast_bf16(good, None, mine, 3, 1, 0)
    assert bool((mine_w == SENT_BF).all())
    call(good, 3, 0b111)  # and the same call with nothing wrong goes through
    assert bool((mine == 0).all()) and _border_intact(mine_w, n)


def test_fp32_rows_on_the_gpu_run_the_reference(gpu):
    x, mask = family("bad_row", 4, 1000)
    x32 = x.float().to(gpu)
    mine = torch.empty(1000, device=gpu)
    cnt = torch.zeros(4, dtype=torch.int64, device=gpu)
    ops.trimmed_reduce_bcast_bf16(x32.view(-1), None, mine, 4, 1, mask, cnt)
    ref, ref_counts = ops.trimmed_mean_reference(x.float(), 1, mask)
    assert torch.equal(bits(mine).cpu(), bits(ref)) and cnt.tolist() == ref_counts.tolist()


def test_averaging_round_end_to_end(gpu):
    """The middle of one robust averaging round on the GPU (a 1-rank group exercises nothing): P peers'
    pseudo-gradient shards stacked as the first all-to-all leaves them, one of them all NaN and one a
    newcomer that does not vote, then the kernel and lsgd_apply. Against the same calls on CPU tensors,
    which is the arithmetic the CPU trainer runs. Everything is bit-equal: the aggregate by the kernel's
    contract, and lsgd_apply with outer_lr = avg_scale = 1 multiplies by +-1 only, so each side rounds
    anchor + avg once."""
    P, n = 5, 4104 * 2
    g = torch.Generator().manual_seed(5)
    anchor = torch.randn(n, generator=g)
    deltas = (0.01 * torch.randn(P, n, generator=g)).to(BF)
    deltas[1] = float("nan")  # the faulty peer
    deltas[4] = 0.0  # a newcomer: all-zero delta, no vote
    mask = robust.mask_of([0, 1, 2, 3], P)
    state = {}
    for dev in ("cpu", gpu):
        a = anchor.clone().to(dev)
        master = (a + 0.5).clone()
        param = torch.zeros(n, dtype=BF, device=dev)
        stack = deltas.clone().to(dev).view(-1)
        avg = torch.empty(n, dtype=BF, device=dev)
        counts = torch.zeros(P, dtype=torch.int64, device=dev)
        ops.trimmed_reduce_bcast_bf16(stack, stack, avg, P, 1, mask, counts)
        ops.lsgd_apply(avg, a, master, param, None, outer_lr=1.0, mu=0.0, nesterov=False, avg_scale=1.0)
        state[str(dev)] = [t.cpu() for t in (avg, a, master, param, counts, stack)]
    (avg_c, a_c, m_c, p_c, c_c, s_c), (avg_g, a_g, m_g, p_g, c_g, s_g) = state["cpu"], state[str(gpu)]
    assert torch.equal(bits(avg_c), bits(avg_g)) and torch.isfinite(avg_g.float()).all()
    assert torch.equal(bits(s_c), bits(s_g))
    assert c_g.tolist() == c_c.tolist() and int(c_g[1]) == n and int(c_g[4]) == 0
    assert torch.equal(a_c, a_g) and torch.equal(m_c, m_g) and torch.equal(bits(p_c), bits(p_g))
    assert torch.equal(a_g, anchor + avg_g.float()) and torch.equal(m_g, a_g)
