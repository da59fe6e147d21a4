"""q8 kernels of compress.hip (encode, reduce, decode) on gfx950: bitwise against the torch
reference run on the same inputs, canaries around every buffer the kernels write."""
import pytest
import torch

from distributedvolunteercomputing_amd.ops._lib import reference_ops
from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor
from tests._q8 import BLOCK, families, simulate_round, unpack

pytestmark = pytest.mark.gpu

SIZES = [1, 127, 128, 129, 8 * 128 + 5, 64 * 1024 + 17]
PEERS = [1, 3, 8]
CANARY_F = -12345.0
CANARY_B = 0xA5
PAD = 64  # canary elements behind every buffer


def _guarded(numel, dtype, dev, canary):
    """(view of the first numel elements, the whole buffer filled with the canary)."""
    big = torch.full((numel + PAD,), canary, dtype=dtype, device=dev)
    return big[:numel], big


def _ref_encode(g, e0, P):
    c = Quant8Compressor(g.numel(), g.device)
    c.e.copy_(e0)
    with reference_ops():
        wire = c.encode(g, P).clone()
    return wire, c.e


@pytest.mark.parametrize("n", SIZES)
def test_q8_encode_bitwise(gpu, n):
    gen = torch.Generator().manual_seed(n)
    e_rand = (0.1 * torch.randn(n, generator=gen)).to(gpu)
    fams = {k: v.to(gpu) for k, v in families(n, seed=n).items()}
    for P in PEERS:
        for dtype in (torch.bfloat16, torch.float32):
            for name, v in fams.items():
                g = v.to(dtype)
                for e0 in (e_rand, torch.zeros_like(e_rand)):  # e = 0: v = g keeps the family's shape
                    ref_wire, ref_e = _ref_encode(g, e0, P)
                    c = Quant8Compressor(n, gpu)
                    c.e, ebig = _guarded(n, torch.float32, gpu, CANARY_F)
                    c.e.copy_(e0)
                    rec = c.layout(P)[2]
                    c._bufs[(P, "wire")], wbig = _guarded(P * rec, torch.uint8, gpu, CANARY_B)
                    wire = c.encode(g, P)
                    tag = (n, P, dtype, name)
                    q, s = unpack(wire, P)
                    rq, rs = unpack(ref_wire, P)
                    assert torch.equal(q, rq), tag
                    assert torch.equal(s.view(torch.int32), rs.view(torch.int32)), tag
                    assert torch.equal(c.e.view(torch.int32), ref_e.view(torch.int32)), tag
                    assert (ebig[n:] == CANARY_F).all() and (wbig[P * rec:] == CANARY_B).all(), tag


def test_q8_encode_unaligned_input(gpu):
    """A gradient view that is not 16-byte aligned takes the element-wise path: same bits."""
    n = 8 * 128 + 5
    torch.manual_seed(5)
    for dtype in (torch.bfloat16, torch.float32):
        gbig = torch.randn(n + 1, device=gpu).to(dtype)
        g = gbig[1:]
        assert g.data_ptr() % 16 != 0
        e0 = 0.1 * torch.randn(n, device=gpu)
        ref_wire, ref_e = _ref_encode(g, e0, 3)
        c = Quant8Compressor(n, gpu)
        c.e.copy_(e0)
        assert torch.equal(c.encode(g, 3), ref_wire) and torch.equal(c.e, ref_e)


def _record(x):
    """The reference's record of one shard holding x (a multiple of 128 elements)."""
    c = Quant8Compressor(x.numel(), x.device)
    with reference_ops():
        return c.encode(x, 1).clone()


@pytest.mark.parametrize("P", [1, 2, 3, 8])
@pytest.mark.parametrize("m", [128, 384, 128 * 33])
def test_q8_reduce_bitwise(gpu, P, m):
    gen = torch.Generator().manual_seed(1000 * P + m)
    variants = ["plain", "zero_peer"] + (["cancel"] if P > 1 else [])
    for variant in variants:
        xs = [(0.01 * (p + 1) * torch.randn(m, generator=gen)).to(gpu) for p in range(P)]
        if variant == "zero_peer":
            xs[P // 2] = torch.zeros(m, device=gpu)
        if variant == "cancel":  # block 0: two opposite peers, nothing from the others
            for p in range(1, P - 1):
                xs[p][:BLOCK] = 0
            xs[P - 1][:BLOCK] = -xs[0][:BLOCK]
        recv = torch.cat([_record(x) for x in xs])
        if variant == "zero_peer":
            zq, zs = unpack(recv, P)
            assert (zq.view(P, m)[P // 2] == 0).all() and (zs.view(P, -1)[P // 2] == 0).all()
        ref = Quant8Compressor(m * P, gpu)
        with reference_ops():
            want = ref.reduce(recv, P).clone()
        c = Quant8Compressor(m * P, gpu)
        assert c.layout(P)[1] == m
        rec = c.layout(P)[2]
        c._bufs[(P, "record")], big = _guarded(rec, torch.uint8, gpu, CANARY_B)
        got = c.reduce(recv, P)
        assert torch.equal(got, want), (P, m, variant)
        assert (big[rec:] == CANARY_B).all(), (P, m, variant)
        if variant == "cancel":
            q, s = unpack(want, 1)
            assert float(s[0]) == 0.0 and (q[:BLOCK] == 0).all()
        if variant == "plain":
            assert (unpack(want, 1)[1] > 0).all()


@pytest.mark.parametrize("n", SIZES)
def test_q8_decode_bitwise(gpu, n):
    fams = families(n, seed=n + 1)
    for P in PEERS:
        for name in ("randn", "wide", "tiny"):
            records, _ = _ref_encode(fams[name].to(gpu), torch.zeros(n, device=gpu), P)
            ref = Quant8Compressor(n, gpu)
            with reference_ops():
                want = ref.decode(records, P).clone()
            c = Quant8Compressor(n, gpu)
            c.out, big = _guarded(n, torch.bfloat16, gpu, 123.0)
            got = c.decode(records, P)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (n, P, name)
            assert (big[n:] == 123.0).all(), (n, P, name)


def _three_rounds(dev, n, P):
    comps = [Quant8Compressor(n, dev) for _ in range(P)]
    res = []
    for rnd in range(3):
        gen = torch.Generator().manual_seed(50 + rnd)
        gs = [(0.01 * torch.randn(n, generator=gen)).to(torch.bfloat16).to(dev) for _ in range(P)]
        outs, _, _ = simulate_round(comps, gs)
        res.append(([o.cpu() for o in outs], [c.e.cpu().clone() for c in comps]))
    return res


def test_q8_whole_compressor_matches_cpu_reference(gpu):
    """Three peers simulated on the GPU (records shuffled with torch copies), three rounds carrying
    e: out and e equal the CPU reference bit for bit every round, and a second GPU run equals the first."""
    n, P = 128 * 33 * 3 + 17, 3
    a = _three_rounds(gpu, n, P)
    b = _three_rounds(gpu, n, P)
    want = _three_rounds(torch.device("cpu"), n, P)
    for rnd in range(3):
        for p in range(P):
            assert torch.equal(a[rnd][0][p].view(torch.int16), want[rnd][0][p].view(torch.int16)), (rnd, p)
            assert torch.equal(a[rnd][1][p].view(torch.int32), want[rnd][1][p].view(torch.int32)), (rnd, p)
            assert torch.equal(a[rnd][0][p].view(torch.int16), b[rnd][0][p].view(torch.int16)), (rnd, p)
            assert torch.equal(a[rnd][1][p], b[rnd][1][p]), (rnd, p)
            assert torch.equal(a[rnd][0][p], a[rnd][0][0])


def test_q8_allreduce_mean_one_peer(gpu):
    """P = 1 is encode then decode into the preallocated output: no collective, no bytes sent."""
    torch.manual_seed(9)
    n = 300_001
    g = (0.01 * torch.randn(n, device=gpu)).to(torch.bfloat16)
    c = Quant8Compressor(n, gpu)
    out = c.allreduce_mean(g, None)
    ref = Quant8Compressor(n, "cpu")
    want = ref.allreduce_mean(g.cpu(), None)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16)) and torch.equal(c.e.cpu(), ref.e)
    assert out.data_ptr() == c.allreduce_mean(g, None).data_ptr() and c.bytes_sent == 0
