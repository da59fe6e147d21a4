"""The gfx950 centered-clipping kernels (csrc/kernels/robust.hip) against the torch definition
(ops/robust.py), bit for bit: result, every row of out, weights, aliasing, borders, repeatability, the
chunk-stride loop, the binding's refusals, and the averaging round's arithmetic end to end."""
import pytest
import torch

from distributedvolunteercomputing_amd import ops
from distributedvolunteercomputing_amd.ops import robust
from tests._cclip import clipping_tau
from tests._robust import FAMILIES, bits, family

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PS = [2, 3, 5, 8, 16]
NS = [8, 4088, 4104, 8 * 4096]  # one vector, one ragged chunk, one chunk plus one vector, whole chunks
PAD = 64  # border elements on each side: 128 B of bf16, 256 B of fp32, so the inside stays 16-byte aligned
SENT = -7.0


def _bordered(n, dtype, dev):
    """(whole, inside): `inside` is n elements with PAD sentinel elements before and after it."""
    whole = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device=dev)
    return whole, whole[PAD:PAD + n]


def _border_intact(whole, n):
    return bool((whole[:PAD] == SENT).all()) and bool((whole[PAD + n:] == SENT).all())


def _expand(ref, P):
    return bits(ref).unsqueeze(0).expand(P, ref.numel())


def test_reference_on_the_gpu_is_the_reference(gpu):
    """The kernel tests build their oracle with the torch definition on the GPU. It is the same oracle: the
    sums run on the device in the documented order, the K square roots and divides in Python floats (correctly
    rounded on any machine), and result, weights, radii and distances have the same bits as on the CPU."""
    for P in (3, 16):
        for name in FAMILIES:
            x, mask = family(name, P, 4104)
            for tau in (0.0, clipping_tau(x, mask)):
                rc, wc, ic = ops.centered_clip_reference(x, mask, tau, 3)
                rg, wg, ig = ops.centered_clip_reference(x.to(gpu), mask, tau, 3)
                tag = (P, name, tau)
                assert torch.equal(bits(rc), bits(rg).cpu()), tag
                assert torch.equal(wc.view(torch.int32), wg.cpu().view(torch.int32)), tag
                assert ic["tau"] == ig["tau"], tag
                assert all(torch.equal(a.view(torch.int32), b.cpu().view(torch.int32))
                           for a, b in zip(ic["dist"], ig["dist"])), tag


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("P", PS)
def test_kernels_match_the_definition_bit_for_bit(gpu, P, n):
    for name in FAMILIES:
        xc, mask = family(name, P, n)
        x = xc.to(gpu)
        for tau in (0.0, clipping_tau(xc, mask)):
            for iters in (1, 3):
                tag = (name, tau, iters)
                ref, wref, _ = ops.centered_clip_reference(x, mask, tau, iters)
                inp_w, inp = _bordered(P * n, BF, gpu)
                inp.copy_(x.view(-1))
                mine_w, mine = _bordered(n, BF, gpu)
                out_w, out = _bordered(P * n, BF, gpu)
                w_w, w = _bordered(P, torch.float32, gpu)
                ops.cclip_reduce_bcast_bf16(inp, out, mine, P, tau, iters, mask, w)
                assert torch.equal(bits(mine), bits(ref)), tag
                assert torch.equal(bits(out).view(P, n), _expand(ref, P)), tag
                assert torch.equal(w.view(torch.int32), wref.view(torch.int32)), (tag, w.tolist(), wref.tolist())
                assert torch.equal(bits(inp), bits(x).view(-1)), tag  # the input is only read
                assert (_border_intact(mine_w, n) and _border_intact(out_w, P * n) and _border_intact(w_w, P)
                        and _border_intact(inp_w, P * n)), tag
                # a second launch on the same input: the same bits (the workspace carries no state)
                mine2 = torch.empty(n, dtype=BF, device=gpu)
                w2 = torch.empty(P, device=gpu)
                ops.cclip_reduce_bcast_bf16(inp, None, mine2, P, tau, iters, mask, w2)
                assert torch.equal(bits(mine2), bits(mine)) and torch.equal(w2.view(torch.int32), w.view(torch.int32)), tag
                # out aliasing in, as in the collective: the same bits in every row
                mine3 = torch.empty(n, dtype=BF, device=gpu)
                ops.cclip_reduce_bcast_bf16(inp, inp, mine3, P, tau, iters, mask, None)
                assert torch.equal(bits(mine3), bits(ref)), tag
                assert torch.equal(bits(inp).view(P, n), _expand(ref, P)) and _border_intact(inp_w, P * n), tag


def test_more_chunks_than_workgroups(gpu):
    """A chunk count above the launcher's workgroup cap by a ragged amount: the chunk-stride loop runs, and
    some workgroups take one chunk more than others."""
    cap = robust.CCLIP_MAX_WORKGROUPS
    assert cap == ops.native().cclip_max_workgroups()
    P, n = 3, (cap + 37) * robust.CCLIP_CHUNK + 1032
    g = torch.Generator().manual_seed(11)
    x = torch.randn(P, n, generator=g).to(BF)
    x[2, ::3] *= 4.0  # one row further out, so that the weights are not all 1
    x = x.to(gpu)
    ref, wref, _ = ops.centered_clip_reference(x, None, 0.0, 2)
    mine_w, mine = _bordered(n, BF, gpu)
    w = torch.empty(P, device=gpu)
    ops.cclip_reduce_bcast_bf16(x.view(-1), None, mine, P, 0.0, 2, None, w)
    assert torch.equal(bits(mine), bits(ref)) and _border_intact(mine_w, n)
    assert torch.equal(w.view(torch.int32), wref.view(torch.int32)) and float(w.min()) < 1.0


def test_one_voter_and_optional_outputs(gpu):
    P, n = 5, 4104
    x, mask = family("bad_row", P, n)
    x = x.to(gpu)
    ref, wref, _ = ops.centered_clip_reference(x, mask, 0.0, 3)
    w = torch.empty(P, device=gpu)
    ops.cclip_reduce_bcast_bf16(x.view(-1), None, None, P, 0.0, 3, mask, w)  # neither out nor mine
    assert torch.equal(w, wref) and float(w[P // 2]) == 0.0
    out = torch.empty(P * n, dtype=BF, device=gpu)
    ops.cclip_reduce_bcast_bf16(x.view(-1), out, None, P, 0.0, 3, mask, None)  # out alone
    assert torch.equal(bits(out).view(P, n), _expand(ref, P)) and torch.isfinite(out.float()).all()
    mine = torch.empty(n, dtype=BF, device=gpu)
    ops.cclip_reduce_bcast_bf16(x.view(-1), None, mine, P, 0.0, 3, mask, None)  # mine alone
    assert torch.equal(bits(mine), bits(ref))
    # one voter, the bad row itself: it comes out unchanged, NaN payloads included
    one = 1 << (P // 2)
    out_w, out1 = _bordered(P * n, BF, gpu)
    ops.cclip_reduce_bcast_bf16(x.view(-1), out1, mine, P, 0.0, 3, one, w)
    assert torch.equal(bits(mine), bits(x[P // 2])) and torch.equal(bits(out1).view(P, n), _expand(x[P // 2], P))
    assert w.tolist() == [1.0 if k == P // 2 else 0.0 for k in range(P)] and _border_intact(out_w, P * n)


def test_binding_refuses_before_anything_is_written(gpu):
    C = ops.native()
    n = 64
    mine_w, mine = _bordered(n, BF, gpu)
    w_w, w = _bordered(16, torch.float32, gpu)

    def call(inp, P, mask, out=None, mine_=mine, weights=None, tau=0.0, iters=2):
        C.cclip_reduce_bcast_bf16(inp, out, mine_, P, mask, tau, iters, weights)

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
        "cpu weights": lambda: call(good, 3, 0b111, weights=torch.zeros(3)),
        "misaligned in": lambda: call(torch.zeros(3 * n + 8, dtype=BF, device=gpu)[4:4 + 3 * n], 3, 0b111),
        "misaligned mine": lambda: call(good, 3, 0b111, mine_=mine_w[PAD + 4:PAD + 4 + n]),
        "short mine": lambda: call(good, 3, 0b111, mine_=mine[:n - 8]),
        "short out": lambda: call(good, 3, 0b111, out=torch.zeros(2 * n, dtype=BF, device=gpu)),
        "fp64 weights": lambda: call(good, 3, 0b111, weights=torch.zeros(3, dtype=torch.float64, device=gpu)),
        "short weights": lambda: call(good, 3, 0b111, weights=w[:2]),
        "negative tau": lambda: call(good, 3, 0b111, weights=w[:3], tau=-1.0),
        "nan tau": lambda: call(good, 3, 0b111, weights=w[:3], tau=float("nan")),
        "inf tau": lambda: call(good, 3, 0b111, weights=w[:3], tau=float("inf")),
        "tau beyond fp32": lambda: call(good, 3, 0b111, weights=w[:3], tau=1e39),
        "iters = 0": lambda: call(good, 3, 0b111, weights=w[:3], iters=0),
        "iters = 9": lambda: call(good, 3, 0b111, weights=w[:3], iters=9),
    }
    for what, fn in bad_calls.items():
        with pytest.raises((RuntimeError, ValueError)):
            fn()
            pytest.fail(f"{what} was accepted")
    torch.cuda.synchronize()
    assert bool((mine_w == SENT).all()) and bool((w_w == SENT).all())
    # the op refuses what the reference refuses, on any device
    with pytest.raises(ValueError):
        ops.cclip_reduce_bcast_bf16(torch.zeros(17 * n, dtype=BF, device=gpu), None, mine, 17, 0.0, 2)
    with pytest.raises(ValueError):
        ops.cclip_reduce_bcast_bf16(good, None, mine, 3, 0.0, 9)
    assert bool((mine_w == SENT).all())
    call(good, 3, 0b111, weights=w[:3])  # and the same call with nothing wrong goes through
    assert bool((mine == 0).all()) and _border_intact(mine_w, n)
    assert w[:3].tolist() == [1.0, 1.0, 1.0] and bool((w[3:] == SENT).all()) and _border_intact(w_w, 16)


def test_fp32_rows_on_the_gpu_run_the_reference(gpu):
    x, mask = family("bad_row", 4, 1000)
    mine = torch.empty(1000, device=gpu)
    w = torch.empty(4, device=gpu)
    ops.cclip_reduce_bcast_bf16(x.float().to(gpu).view(-1), None, mine, 4, 0.0, 2, mask, w)
    ref, wref, _ = ops.centered_clip_reference(x.float(), mask, 0.0, 2)
    assert torch.equal(bits(mine).cpu(), bits(ref)) and torch.equal(w.cpu(), wref)


def test_averaging_round_end_to_end(gpu):
    """The middle of one cclip averaging round on the GPU: P peers' pseudo-gradient shards stacked as the first
    all-to-all leaves them, one of them all NaN and one a newcomer that does not vote, then the kernels and
    lsgd_apply. Against the same calls on CPU tensors, which is the arithmetic the CPU trainer runs. Everything
    is bit-equal: the aggregate by the kernels' contract, and lsgd_apply with outer_lr = avg_scale = 1 multiplies
    by +-1 only, so each side rounds anchor + avg once."""
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
        w = torch.zeros(P, device=dev)
        ops.cclip_reduce_bcast_bf16(stack, stack, avg, P, 0.0, 3, mask, w)
        ops.lsgd_apply(avg, a, master, param, None, outer_lr=1.0, mu=0.0, nesterov=False, avg_scale=1.0)
        state[str(dev)] = [t.cpu() for t in (avg, a, master, param, w, stack)]
    (avg_c, a_c, m_c, p_c, w_c, s_c), (avg_g, a_g, m_g, p_g, w_g, s_g) = state["cpu"], state[str(gpu)]
    assert torch.equal(bits(avg_c), bits(avg_g)) and torch.isfinite(avg_g.float()).all()
    assert torch.equal(bits(s_c), bits(s_g))
    assert torch.equal(w_c, w_g) and float(w_g[1]) == 0.0 and float(w_g[4]) == 0.0 and int((w_g == 1.0).sum()) >= 2
    assert torch.equal(a_c, a_g) and torch.equal(m_c, m_g) and torch.equal(bits(p_c), bits(p_g))
    assert torch.equal(a_g, anchor + avg_g.float()) and torch.equal(m_g, a_g)
