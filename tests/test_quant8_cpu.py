"""q8 (8-bit block quantisation with error feedback) on the torch reference: the codec contract,
error-feedback conservation, the three stages over simulated peers, real gloo collectives, both
trainers, the elastic rollback and the train CLI."""
import time

import pytest
import torch

from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor
from tests import _mp
from tests._q8 import BLOCK, HALF, TINY, families, simulate_round, unpack


def _blocks(x: torch.Tensor, L: int) -> torch.Tensor:
    """x [n] zero-padded to L as [L / 128, 128]."""
    v = torch.zeros(L, dtype=x.dtype)
    v[: x.numel()] = x
    return v.view(-1, BLOCK)


# ------------------------------------------------------------------------------ codec contract
@pytest.mark.parametrize("n", [1, 127, 128, 129, 128 * 5 + 3])
def test_codec_contract(n):
    """|q| <= 127, finite output, scale == 0 implies all codes 0, and |v - dec| <= scale (0.5 + 2^-16)
    per element of every block that is sent. A block below 2^-100 sends nothing by the codec's own
    definition (scale 0, codes 0), so for it the bound reads: its content stays in the error
    feedback unchanged."""
    for name, v in families(n).items():
        c = Quant8Compressor(n, "cpu")
        wire = c.encode(v, 1)
        L = c.layout(1)[0]
        q, scale = unpack(wire, 1)
        assert q.numel() == L and scale.numel() == L // BLOCK, name
        assert int(q.to(torch.int32).abs().max()) <= 127, name
        dec = q.float().view(-1, BLOCK) * scale.unsqueeze(1)
        assert torch.isfinite(dec).all() and torch.isfinite(scale).all() and torch.isfinite(c.e).all(), name
        assert (scale >= 0).all() and (q.view(-1, BLOCK)[scale == 0] == 0).all(), name
        vb = _blocks(v, L)
        sent = vb.abs().amax(dim=1) >= TINY
        assert torch.equal(sent, scale > 0), name
        err = (vb.double() - dec.double()).abs()
        assert (err[sent] <= scale[sent].double().unsqueeze(1) * HALF).all(), name
        assert torch.equal(dec[~sent], torch.zeros_like(dec[~sent])), name
        # the error feedback holds exactly what was not sent; padding beyond n encodes as zeros
        assert torch.equal(c.e, (vb - dec).view(-1)[:n]), name
        assert (q[n:] == 0).all(), name
        assert torch.equal(c.decode_f32(wire, 1), dec.view(-1)[:n]), name


def test_error_feedback_conservation():
    """50 rounds at one peer: sum g - sum dec - e stays at fp32 rounding level (fp64 bookkeeping,
    dec taken before the bf16 output rounding)."""
    torch.manual_seed(1)
    n = 8192
    c = Quant8Compressor(n, "cpu")
    sg = torch.zeros(n, dtype=torch.float64)
    sd = torch.zeros(n, dtype=torch.float64)
    for _ in range(50):
        g = (0.01 * torch.randn(n)).to(torch.bfloat16)
        wire = c.encode(g, 1)
        sg += g.double()
        sd += c.decode_f32(wire, 1).double()
    drift = float((sg - sd - c.e.double()).abs().max())
    print(f"[q8 conservation] drift {drift:.3e} of max|sum g| {float(sg.abs().max()):.3e}")
    assert drift <= 1e-6 * float(sg.abs().max())


# ------------------------------------------------------------------------------ three stages
def _inputs(kind: str, n: int, P: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(P):
        x = 0.01 * torch.randn(n, generator=g)
        if kind == "wide":
            x = x * torch.exp(4 * torch.randn(n, generator=g))
        elif kind == "sparse":
            x = x * (torch.rand(n, generator=g) >= 0.9)
        out.append(x)
    return out


@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_three_stages_simulated_peers(P):
    """P compressors in one process: identical result on every peer, within the two quantisations'
    half code units (plus the bf16 output rounding) of the fp64 mean."""
    worst = 0.0
    for n in (1, 127, 129, 128 * 7 + 5, 128 * 33 * P + 17):
        for kind in ("plain", "wide", "sparse"):
            gs = _inputs(kind, n, P, seed=n + P)
            comps = [Quant8Compressor(n, "cpu") for _ in range(P)]
            outs, wires, gathered = simulate_round(comps, gs)
            for o in outs[1:]:
                assert torch.equal(o, outs[0]), (n, kind)
            L = comps[0].layout(P)[0]
            s1 = torch.stack([unpack(w, P)[1] for w in wires]).double().mean(dim=0)
            s2 = unpack(gathered, P)[1].double() if P > 1 else torch.zeros_like(s1)
            q = (HALF * (s1 + s2)).unsqueeze(1).expand(-1, BLOCK).reshape(-1)[:n]
            mean = torch.stack(gs).double().mean(dim=0)
            bound = q + 2.0 ** -8 * (mean.abs() + q)
            err = (outs[0].double() - mean).abs()
            assert (err <= bound).all(), (n, kind, float((err / bound.clamp_min(1e-300)).max()))
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert L % (BLOCK * P) == 0 and L >= n
    print(f"[q8 three stages] P={P} worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------ real collectives
_N_COLL = 128 * 7 + 5


def _coll_input(rank: int, rnd: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 * rnd + rank)
    return (0.01 * torch.randn(_N_COLL, generator=g)).to(torch.bfloat16)


def _coll_worker(rank, world, port):
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    store = _mp.make_store(rank, world, port)
    grp = PeerGroup(store, rank, world, "gloo")
    c = Quant8Compressor(_N_COLL, "cpu")
    outs = []
    for rnd in range(2):
        outs.append(c.allreduce_mean(_coll_input(rank, rnd), grp).view(torch.int16).tolist())
    ptr_same = c.allreduce_mean(_coll_input(rank, 2), grp).data_ptr() == c.out.data_ptr()
    grp.barrier()
    return {"outs": outs, "e": c.e.tolist(), "bytes": c.bytes_sent, "reused": ptr_same}


@pytest.mark.parametrize("P", [3, 2])
def test_real_collectives_match_simulation(P):
    res = _mp.run(_coll_worker, P)
    comps = [Quant8Compressor(_N_COLL, "cpu") for _ in range(P)]
    rec = comps[0].layout(P)[2]
    for rnd in range(2):
        outs, _, _ = simulate_round(comps, [_coll_input(r, rnd) for r in range(P)])
        for r in range(P):
            assert res[r]["outs"][rnd] == outs[r].view(torch.int16).tolist(), (rnd, r)
    simulate_round(comps, [_coll_input(r, 2) for r in range(P)])
    for r in range(P):
        assert res[r]["e"] == comps[r].e.tolist()
        assert res[r]["bytes"] == 3 * 2 * (P - 1) * rec and res[r]["reused"]
    L = comps[0].layout(P)[0]
    assert 2 * (P - 1) * rec * P == 2 * (P - 1) * (L + L // 32)  # (P-1)/P (L + L/32) per collective


# ------------------------------------------------------------------------------ training
def _mlp_q8_trainer(group=None, membership=None, H=2):
    from distributedvolunteercomputing_amd.models.mlp import MLP
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer

    cfg = LocalSGDConfig(H=H, lr=0.05, weight_decay=0.0, max_grad_norm=0.0, comm_dtype=torch.bfloat16)
    tr = LocalSGDTrainer(MLP(seed=0), cfg, group=group, membership=membership, device="cpu")
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    return tr


def _local_sgd_worker(rank, world, port):
    from distributedvolunteercomputing_amd.models.mlp import synthetic_mnist
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    store = _mp.make_store(rank, world, port)
    g = PeerGroup(store, rank, world, "gloo")
    tr = _mlp_q8_trainer(group=g)
    tr.cfg.algo = "rccl"
    x, y = synthetic_mnist(512, seed=rank)
    losses = []
    for i in range(12):
        b = slice((i % 8) * 64, (i % 8 + 1) * 64)
        losses.append(float(tr.step(x[b], y[b]).extra["loss_t"]))
    a = tr.anchor.clone()
    g.allreduce_(a)
    same = torch.equal(a / world, tr.anchor)
    g.barrier()
    return {"first": losses[0], "last": losses[-1], "same": same, "syncs": tr.sync_count,
            "bytes": tr.compressor.bytes_sent, "ef": float(tr.compressor.e.abs().sum())}


def test_local_sgd_q8():
    res = _mp.run(_local_sgd_worker, 2)
    for r in res.values():
        assert r["same"] and r["syncs"] == 6
        assert r["last"] < r["first"], r
        assert r["bytes"] > 0 and r["ef"] > 0


def _sharded_worker(rank, world, port):
    from distributedvolunteercomputing_amd.models.mlp import MLP, synthetic_mnist
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup
    from distributedvolunteercomputing_amd.parallel.zero import ShardedConfig, ShardedDPTrainer

    store = _mp.make_store(rank, world, port)
    g = PeerGroup(store, rank, world, "gloo")
    m = MLP(seed=0)
    numel = sum(p.numel() for p in m.parameters())
    tr = ShardedDPTrainer(m, ShardedConfig(lr=1e-2, weight_decay=0.0), group=g, device="cpu")
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    assert tr.flat.numel >= numel
    x, y = synthetic_mnist(256, seed=rank)
    losses = [float(tr.step(x[i * 16:(i + 1) * 16], y[i * 16:(i + 1) * 16])) for i in range(10)]
    p = tr.flat.param.float().clone()
    g.allreduce_(p)
    same = torch.equal(p / world, tr.flat.param.float())
    g.barrier()
    return {"same": same, "first": losses[0], "last": losses[-1], "bytes": tr.compressor.bytes_sent}


def test_sharded_trainer_q8():
    res = _mp.run(_sharded_worker, 2)
    for r in res.values():
        assert r["same"], r
        assert r["bytes"] > 0 and r["last"] == r["last"]


# ------------------------------------------------------------------------------ elastic
def _elastic_worker(rank, world, port, drop_rank):
    from distributedvolunteercomputing_amd.models.mlp import synthetic_mnist
    from distributedvolunteercomputing_amd.parallel.elastic import ElasticMembership

    store = _mp.make_store(rank, world, port)
    mem = ElasticMembership(store, rank, backend="gloo", lease_s=1.0, heartbeat_s=0.1)
    mem.bootstrap(list(range(world)))
    tr = _mlp_q8_trainer(membership=mem, H=2)
    x, y = synthetic_mnist(256, seed=rank)
    i = 0
    while not (mem.gen == 1 and mem.round >= 2) and i < 2000:
        if mem.gen < 1 and i > 200:
            time.sleep(0.01)  # waiting for the membership change: slow down, keep the rounds going
        b = slice((i % 8) * 32, (i % 8 + 1) * 32)
        tr.step(x[b], y[b])
        i += 1
        if rank == drop_rank and i == 5:
            mem.stop_heartbeat()  # simulated crash: vanish without a word
            return {"dropped": True}
    store.set(f"done/{rank}", "1")
    if rank == 0:  # the store lives in rank 0: keep it up until every live peer is done
        t0 = time.time()
        while not store.check([f"done/{m}" for m in mem.members]) and time.time() - t0 < 60:
            time.sleep(0.02)
    ev = [e for e in mem.events if e["event"] in ("regroup", "joined")]
    layouts = sorted({k[0] for k in tr.compressor._bufs})
    return {"members": mem.members, "events": ev, "anchor_sum": float(tr.anchor.sum()),
            "bytes": tr.compressor.bytes_sent, "layouts": layouts}


def test_elastic_drop_continues_on_survivors_q8():
    res = _mp.run(_elastic_worker, 3, 2, timeout=120, expect_exit=(2,))
    for r in (0, 1):
        assert res[r]["members"] == [0, 1]
        assert any(e["dropped"] == [2] for e in res[r]["events"])
        # the 3-peer layout's buffers were dropped when the 2-peer one was allocated
        assert res[r]["bytes"] > 0 and res[r]["layouts"] == [2]
    assert abs(res[0]["anchor_sum"] - res[1]["anchor_sum"]) < 1e-4


def test_rollback_gives_fresh_compressor_bits():
    """snapshot -> allreduce_mean -> restore -> allreduce_mean equals a fresh compressor holding the
    same error feedback; restore also drops the buffers a collective may still own."""
    torch.manual_seed(3)
    n = 128 * 7 + 5
    c = Quant8Compressor(n, "cpu")
    c.allreduce_mean((0.01 * torch.randn(n)).to(torch.bfloat16), None)  # leaves a non-zero e
    e0 = c.e.clone()
    assert float(e0.abs().sum()) > 0
    snap = c.snapshot()
    old_wire = c._buf(1, "wire")
    c.allreduce_mean((0.01 * torch.randn(n)).to(torch.bfloat16), None)  # the round that gets aborted
    assert not torch.equal(c.e, e0) and torch.equal(snap["e"], e0)
    c.restore(snap)
    g = (0.01 * torch.randn(n)).to(torch.bfloat16)
    out = c.allreduce_mean(g, None).clone()
    assert c._buf(1, "wire").data_ptr() != old_wire.data_ptr()
    fresh = Quant8Compressor(n, "cpu")
    fresh.load_state_dict({"ef": e0})
    assert torch.equal(out, fresh.allreduce_mean(g, None))
    assert torch.equal(c.e, fresh.e) and torch.equal(c.state_dict()["ef"], fresh.e)


# ------------------------------------------------------------------------------ interface
@pytest.mark.parametrize("trainer", ["localsgd", "sharded"])
def test_train_cli_q8(trainer, monkeypatch):
    from distributedvolunteercomputing_amd.jobs import train
    from distributedvolunteercomputing_amd.parallel import compression

    a = train.parse(["--compression", "q8"])
    assert a.compression == "q8"
    built = []

    class Recording(Quant8Compressor):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            built.append(self)

    monkeypatch.setattr(compression, "Quant8Compressor", Recording)
    rc = train.main(["--model", "mlp", "--trainer", trainer, "--steps", "2", "--H", "1", "--batch", "16",
                     "--compression", "q8", "--backend", "gloo", "--peer-id", "0", "--world", "1",
                     "--store-port", str(_mp.free_port()), "--log-every", "1"])
    assert rc == 0 and len(built) == 1
    assert built[0].bytes_per_element == 1.03125
    if trainer == "sharded":  # one peer still quantises its gradient (as top-k compresses at one peer)
        assert float(built[0].e.abs().sum()) > 0
