"""Compact AdamW state (fp8 e4m3 m, fp16 v, one power-of-two exponent per 32 elements): the torch
definition of the codec, training with it, checkpoints across modes and peer counts, and the sharded
trainer's replicas and re-shard. No GPU.

Single-peer training, measured here (MLP, 200 steps, final loss = mean of the last 20 steps):
see profiles/opt_state_compact.txt.
"""
import os

import pytest
import torch

from distributedvolunteercomputing_amd.ops import optim as O
from distributedvolunteercomputing_amd.ops.optim import CompactState
from tests import _mp
from tests._optstate import adversarial

N = 64000
KW = dict(beta1=0.9, beta2=0.95, eps=1e-8, wd=0.1)


@pytest.fixture(scope="module")
def adv():
    m, v = adversarial(N, seed=0)
    return m, v, CompactState.from_fp32(m, v)


def _block(t):
    return t.reshape(-1, O.CS_BLOCK)


# ------------------------------------------------------------------ codec properties
def test_codec_reencode_is_identity(adv):
    _, _, st = adv
    m, v = st.to_fp32()
    assert torch.isfinite(m).all() and torch.isfinite(v).all()
    again = CompactState.from_fp32(m, v)
    for name, a, b in zip(st.FIELDS, st.arrays(), again.arrays()):
        assert torch.equal(a, b), name
    assert st.nbytes == N + 2 * N + 2 * (N // 32)


def test_codec_m_error_bound(adv):
    m, _, st = adv
    dec, _ = st.to_fp32()
    live = (st.m_exp > 0)[:, None].expand(-1, O.CS_BLOCK)
    assert live.any() and not live.all()
    e = st.m_exp.double() - 127
    scaled = _block(m).double().abs() * torch.exp2(-e)[:, None]
    err = (_block(m).double() - _block(dec).double()).abs()
    # round to nearest: half a step of a 3-bit mantissa, or half the subnormal step 2^-9 of the scaled value;
    # an element scaled into (240, 256) is clamped to 240: at most 16 / 256 of it
    bound = torch.where(scaled > 240, 2.0 ** -3.9 * _block(m).double().abs(),
                        2.0 ** -4 * _block(m).double().abs() + torch.exp2(e - 10)[:, None])
    assert (scaled > 240).any()
    assert bool((err[live] <= bound[live]).all())
    assert bool((scaled[live].reshape(-1, O.CS_BLOCK).amax(1) >= 128).all())  # the maximum scales into [128, 256)


def test_codec_v_error_bound_and_floor(adv):
    _, v, st = adv
    _, dec = st.to_fp32()
    live = (st.v_exp > 0)[:, None].expand(-1, O.CS_BLOCK)
    e = st.v_exp.double() - 127
    x, d = _block(v).double(), _block(dec).double()
    floor = torch.exp2(e - 24)[:, None].expand_as(x)
    # fp16 round to nearest: 2^-11 relative (also for the maximum clamped to 32752), half the subnormal
    # step below 2^-14; anything positive below the floor decodes to the floor
    near = (x - d).abs() <= 2.0 ** -11 * x + torch.exp2(e - 25)[:, None]
    at_floor = (d == floor) & (x < floor)
    assert at_floor[live].any()
    assert bool((near | at_floor)[live].all())
    assert bool((d[live & (x > 0)] > 0).all())  # no positive v decodes to 0 in a live block
    assert bool((d[live & (x == 0)] == 0).all())


def test_codec_dead_blocks_decode_to_zero(adv):
    m, v, st = adv
    dm, dv = st.to_fp32()
    dead_m = _block(m).abs().amax(1) < 2.0 ** -100
    dead_v = _block(v).abs().amax(1) < 2.0 ** -100
    assert dead_m.sum() >= 2 * (N // 32 // 16) and (_block(m)[dead_m] != 0).any()  # zero blocks and tiny ones
    assert torch.equal(st.m_exp == 0, dead_m) and torch.equal(st.v_exp == 0, dead_v)
    assert _block(st.m_code)[dead_m].eq(0).all() and _block(st.v_half)[dead_v].eq(0).all()
    assert _block(dm)[dead_m].eq(0).all() and _block(dv)[dead_v].eq(0).all()


@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_zero_state_steps_like_fresh_fp32(max_norm):
    torch.manual_seed(1)
    n = 64 * 37
    p = torch.randn(n).to(torch.bfloat16)
    g = (torch.randn(n) * 0.1).to(torch.bfloat16)
    pa, pb, ma, mb = p.clone(), p.clone(), p.float(), p.float()
    m, v = torch.zeros(n), torch.zeros(n)
    st = CompactState.zeros(n, "cpu")
    oa, ob = O.new_ostate("cpu", 1e-2), O.new_ostate("cpu", 1e-2)
    O.adamw_step(pa, g, ma, m, v, oa, n_decay=64 * 20, max_norm=max_norm, **KW)
    O.adamw_step_compact(pb, g, mb, st, ob, n_decay=64 * 20, max_norm=max_norm, **KW)
    assert torch.equal(ma, mb) and torch.equal(pa, pb) and torch.equal(oa, ob)
    assert st.equal(CompactState.from_fp32(m, v))


def test_state_rejects_ranges_off_the_block():
    with pytest.raises(ValueError):
        CompactState.zeros(40, "cpu")
    with pytest.raises(ValueError):
        CompactState.zeros(64, "cpu").narrow(8, 40)


# ------------------------------------------------------------------ single-peer training
def _train(seed, opt_state, steps=200):
    from distributedvolunteercomputing_amd.models.mlp import MLP, synthetic_mnist
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer

    # the MLP set-up of test_training_dist_cpu.py at Adam's usual lr of 1e-3: at that file's lr = 0.05 the
    # separable data drives the fp32 loss to exactly 0.0 on every seed, which would compare nothing
    cfg = LocalSGDConfig(H=2, lr=1e-3, weight_decay=0.0, max_grad_norm=0.0, comm_dtype=torch.float32,
                         opt_state=opt_state)
    tr = LocalSGDTrainer(MLP(seed=seed), cfg, device="cpu")
    x, y = synthetic_mnist(512, seed=seed)
    losses = []
    for i in range(steps):
        b = slice((i % 8) * 64, (i % 8 + 1) * 64)
        losses.append(float(tr.step(x[b], y[b]).extra["loss_t"]))
    return sum(losses[-20:]) / 20, losses[0]


def test_single_peer_training_within_seed_noise():
    """Each seed's compact run must end within 3 seed-to-seed standard deviations of its fp32 twin."""
    seeds = range(5)
    fp32 = [_train(s, "fp32") for s in seeds]
    comp = [_train(s, "compact") for s in seeds]
    f = torch.tensor([a for a, _ in fp32], dtype=torch.float64)
    c = torch.tensor([a for a, _ in comp], dtype=torch.float64)
    mean, std = f.mean().item(), f.std().item()
    print(f"\nfp32 final loss per seed {f.tolist()} mean {mean:.6g} std {std:.6g}")
    print(f"compact final loss per seed {c.tolist()} mean {c.mean().item():.6g}; first-step loss {fp32[0][1]:.4f}")
    assert all(last < 0.5 * first for last, first in fp32 + comp)  # both modes train
    assert std > 0 and f.min().item() > 0  # a loss that underflowed to 0 would compare nothing
    for s in seeds:
        assert abs(c[s].item() - f[s].item()) <= 3 * std, (s, c[s].item(), f[s].item(), std)


@pytest.mark.parametrize("betas", [(0.95, 0.95), (0.9, 0.9995)])
def test_compact_refuses_slow_betas(betas):
    from distributedvolunteercomputing_amd.models.mlp import MLP
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer
    from distributedvolunteercomputing_amd.parallel.zero import ShardedConfig, ShardedDPTrainer

    with pytest.raises(ValueError, match="stops moving"):
        LocalSGDTrainer(MLP(seed=0), LocalSGDConfig(betas=betas, opt_state="compact"), device="cpu")
    with pytest.raises(ValueError, match="stops moving"):
        ShardedDPTrainer(MLP(seed=0), ShardedConfig(betas=betas, opt_state="compact"), device="cpu")
    LocalSGDTrainer(MLP(seed=0), LocalSGDConfig(betas=betas), device="cpu")  # fp32 takes any betas
    with pytest.raises(ValueError):
        LocalSGDTrainer(MLP(seed=0), LocalSGDConfig(opt_state="fp16"), device="cpu")


# ------------------------------------------------------------------ checkpoints
def _sharded(opt_state, group=None, replicas=2):
    from distributedvolunteercomputing_amd.models.mlp import MLP
    from distributedvolunteercomputing_amd.parallel.zero import ShardedConfig, ShardedDPTrainer

    cfg = ShardedConfig(lr=1e-2, weight_decay=0.0, replicas=replicas, opt_state=opt_state)
    return ShardedDPTrainer(MLP(seed=0), cfg, group=group, device="cpu")


def _steps(tr, rank, k, start=0):
    from distributedvolunteercomputing_amd.models.mlp import synthetic_mnist

    x, y = synthetic_mnist(32 * (start + k), seed=rank)
    for i in range(start, start + k):
        tr.step(x[i * 32:(i + 1) * 32], y[i * 32:(i + 1) * 32])


def _ckpt_writer(rank, world, port, root):
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup
    from distributedvolunteercomputing_amd.utils.checkpoint import save_checkpoint

    g = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo", generation=0)
    tr = _sharded("compact", group=g, replicas=1)
    _steps(tr, rank, 3)
    save_checkpoint(tr, root, 3, peer_id=rank, is_writer=rank == 0, members=[0, 1], barrier=g.barrier)
    return {"range": tr.prim, "master": tr.master.numpy().tobytes(),
            **{f: t.numpy().tobytes() for f, t in zip(tr.cs.FIELDS, tr.cs.arrays())}}


def test_checkpoint_compact_to_other_peer_count_and_to_fp32(tmp_path):
    from distributedvolunteercomputing_amd.utils.checkpoint import ShardReader, latest

    root = str(tmp_path / "ck")
    out = _mp.run(_ckpt_writer, 2, root, timeout=120)
    reader = ShardReader(latest(root))
    one = _sharded("compact")  # written by 2 peers, restored by 1
    one.restore(reader)
    assert one.prim == (0, one.flat.numel) and out[0]["range"][1] == out[1]["range"][0]
    for f, t in zip(one.cs.FIELDS, one.cs.arrays()):
        assert t.numpy().tobytes() == out[0][f] + out[1][f], f
    assert one.master.numpy().tobytes() == out[0]["master"] + out[1]["master"]
    # the same file into an fp32 trainer: its moments are the decoded values
    ref = _sharded("fp32")
    ref.restore(reader)
    m, v = one.cs.to_fp32()
    assert torch.equal(ref.m, m) and torch.equal(ref.v, v) and torch.equal(ref.master, one.master)
    assert m.abs().max() > 0 and v.max() > 0
    _steps(one, 0, 1, start=3)  # and it trains on


def test_checkpoint_fp32_restores_into_compact(tmp_path):
    from distributedvolunteercomputing_amd.models.mlp import MLP
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer
    from distributedvolunteercomputing_amd.utils.checkpoint import ShardReader, latest, save_checkpoint

    root = str(tmp_path / "ck")
    src = _sharded("fp32")
    _steps(src, 0, 3)
    save_checkpoint(src, root, 3, peer_id=0, is_writer=True, members=[0])
    with open(os.path.join(latest(root), "manifest.json")) as f:
        assert '"vcx-ckpt-v1"' in f.read()
    reader = ShardReader(latest(root))
    dst = _sharded("compact")
    dst.restore(reader)
    assert dst.cs.equal(CompactState.from_fp32(src.m, src.v)) and torch.equal(dst.master, src.master)
    assert dst.m is None and dst.state_bytes() == 4 * dst.flat.numel + dst.cs.nbytes
    # the local-SGD trainer reads the same file in compact mode, and writes fp32 moments back
    loc = LocalSGDTrainer(MLP(seed=0), LocalSGDConfig(opt_state="compact"), device="cpu")
    loc.restore(reader)
    assert loc.cstate.equal(dst.cs) and set(loc.cstate.FIELDS) <= set(loc.state_tensors())
    lo, hi, t = loc.checkpoint_slice()
    m, v = dst.cs.to_fp32()
    assert (lo, hi) == (0, loc.flat.numel) and torch.equal(t["m"], m) and torch.equal(t["v"], v)


# ------------------------------------------------------------------ three peers: replicas and re-shard
def _gather(g, n, lo, hi, t):
    """The global array from the primaries' pieces (exact: every element has one non-zero contribution)."""
    full = torch.zeros(n, dtype=torch.float32)
    full[lo:hi] = t.float()
    return g.allreduce_(full)


def _three_peers(rank, world, port):
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    store = _mp.make_store(rank, world, port)
    g = PeerGroup(store, rank, world, "gloo", generation=0)
    tr = _sharded("compact", group=g, replicas=2)
    _steps(tr, rank, 3)
    n, B = tr.flat.numel, O.CS_BLOCK
    lo, hi = tr.prim
    full = CompactState(_gather(g, n, lo, hi, tr.cs.m_code).to(torch.uint8),
                        _gather(g, n // B, lo // B, hi // B, tr.cs.m_exp).to(torch.uint8),
                        _gather(g, n, lo, hi, tr.cs.v_half).to(torch.float16),
                        _gather(g, n // B, lo // B, hi // B, tr.cs.v_exp).to(torch.uint8))
    full_master = _gather(g, n, lo, hi, tr.master)
    assert len(tr.reps) == 2 and full.m_exp.max() > 0 and full.v_exp.max() > 0
    for rep in tr.reps:  # every replica equals its primary, bit for bit
        a, b = rep["range"]
        assert rep["cs"].equal(full.narrow(a, b)), (rank, a, b)
        assert torch.equal(rep["master"], full_master[a:b])
    size = lambda h: 4 * h["master"].numel() + sum(t.numel() * t.element_size() for t in h["cs"].arrays())  # noqa: E731
    assert tr.state_bytes() == sum(size(h) for h in tr._held()) < 12 * 3 * (hi - lo)
    res = {"rank": rank}
    if rank < 2:
        ng = PeerGroup(store, rank, 2, "gloo", generation=1, members=[0, 1])
        tr.reshard(ng)
        m, v = full.to_fp32()
        held = tr._held()
        assert len(held) == 2
        for h in held:  # the old holders' decoded state, encoded over the new ranges
            a, b = h["range"]
            assert h["cs"].equal(CompactState.from_fp32(m[a:b], v[a:b])), (rank, a, b)
            assert h["cs"].equal(full.narrow(a, b)) and torch.equal(h["master"], full_master[a:b])
        _steps(tr, rank, 2, start=3)
        assert tr.state_bytes() == sum(size(h) for h in tr._held())
        res["bytes_changed"] = tr.reshard_events[-1]["bytes_changed"]
    return res


def test_three_peers_replicas_bit_identical_then_reshard():
    out = _mp.run(_three_peers, 3, timeout=120)
    assert all("bytes_changed" in out[r] for r in (0, 1))
