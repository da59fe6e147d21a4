"""Centered clipping (cclip) on the torch reference: the rule's structure, its summation order, what it buys
over the coordinate-wise rules, real gloo collectives, local-SGD training next to a wrong peer, the refusals."""
import hashlib
import json
import math

import numpy as np
import pytest
import torch

from distributedvolunteercomputing_amd import ops
from distributedvolunteercomputing_amd.ops import robust
from tests import _mp
from tests._cclip import ATTACKS, attacked, clipping_tau, honest_rows, rel_l2, tree_distance
from tests._robust import FAMILIES, bits, family

BF = torch.bfloat16


# ------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("P", [3, 8, 16])
@pytest.mark.parametrize("name", FAMILIES)
def test_structure_of_the_reference(name, P):
    n, L = 4104, 3
    x, mask = family(name, P, n)
    live = [k for k in range(P) if (mask >> k) & 1]
    K = len(live)
    row_finite = torch.isfinite(x.float()).all(dim=1)
    start = ops.trimmed_mean_reference(x, (K - 1) // 2, mask)[0]
    assert torch.isfinite(start.float()).all()  # these families leave the median finite everywhere
    for tau in (0.0, 0.5 * clipping_tau(x, mask)):
        res, w, info = ops.centered_clip_reference(x, mask, tau, L)
        assert res.dtype == BF and w.dtype == torch.float32 and w.shape == (P,)
        assert len(info["tau"]) == L and len(info["dist"]) == L and len(info["centres"]) == L + 1
        assert torch.equal(info["centres"][0], start.float())
        for k in range(P):
            if k not in live or not row_finite[k]:
                assert float(w[k]) == 0.0, (tau, k)
            else:
                assert 0.0 <= float(w[k]) <= 1.0, (tau, k)
        assert torch.isfinite(res.float()).all(), tau
        if tau == 0.0:
            assert all(math.isfinite(t) for t in info["tau"])
            assert int((w == 1.0).sum()) >= (K - 1) // 2 + 1, w
        else:
            assert info["tau"] == [float(torch.tensor(tau, dtype=torch.float32))] * L
        for l in range(L):  # every update moves the centre by at most tau_l in l2
            step = float((info["centres"][l + 1].double() - info["centres"][l].double()).norm())
            print(f"[cclip structure] {name} P={P} tau={tau:.4g} l={l}: step {step:.6g} tau_l {info['tau'][l]:.6g}")
            assert step <= info["tau"][l] * (1 + 1e-4), (tau, l)
    _, w, _ = ops.centered_clip_reference(x, mask, 1e30, L)
    assert w.tolist() == [1.0 if (k in live and row_finite[k]) else 0.0 for k in range(P)]


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_one_voter_is_the_identity_and_two_voters_work(dtype):
    x, _ = family("bad_row", 4, 520)
    x = x.to(dtype)
    res, w, info = ops.centered_clip_reference(x, 0b0100, 0.0, 3)  # the one voter is the bad row: still unchanged
    assert torch.equal(bits(res), bits(x[2])) and w.tolist() == [0.0, 0.0, 1.0, 0.0] and info["tau"] == []
    res, w, info = ops.centered_clip_reference(x, 0b1001, 0.0, 2)
    mean = ops.trimmed_mean_reference(x, 0, 0b1001)[0]
    # two voters: the start is their mean and tau is the smaller of two nearly equal distances
    assert torch.isfinite(res.float()).all() and w[1] == 0 and w[2] == 0 and float(w.max()) == 1.0
    assert min(float(w[0]), float(w[3])) > 0.9 and info["tau"][0] == float(info["dist"][0][[0, 3]].min()) > 0
    assert rel_l2(res.float(), mean.float()) < 0.02


def test_fp32_rows_and_the_canonical_nan():
    x, mask = family("bad_row", 2, 264)  # two voters, one of them bad: the mean start is not finite there
    for dtype, canon in ((BF, 0x7FC0), (torch.float32, 0x7FC00000)):
        res, w, _ = ops.centered_clip_reference(x.to(dtype), mask, 0.0, 2)
        nan = torch.isnan(res)
        assert res.dtype == dtype and bool(nan.any()) and w.tolist() == [0.0, 0.0]
        assert (bits(res)[nan].to(torch.int64) & (0xFFFF if dtype == BF else 0xFFFFFFFF) == canon).all()


# ------------------------------------------------------------------------------ the summation order
def test_the_summation_order_is_the_documented_one():
    m = 4096
    u = torch.full((m,), 2.0)
    u[0] = 8192.0  # rows 0 and u: the start is u / 2, both rows are e = -+u / 2 away, e * e = 2^24, 1, 1, ...
    x = torch.stack([torch.zeros(m), u])
    e = (u / 2).numpy()
    tree = tree_distance(e)
    running = np.float32(0.0)
    for q in (e * e).tolist():
        running = np.float32(running + np.float32(q))
    # slot 0 drops its 15 units next to 2^24, the other 255 slots bring 16 each and the tree keeps them all
    assert float(running) == 2.0 ** 24 and float(tree) == 2.0 ** 24 + 255 * 16
    _, _, info = ops.centered_clip_reference(x, None, 0.0, 1)
    assert info["dist"][0].tolist() == [float(np.sqrt(tree))] * 2 and float(np.sqrt(tree)) != 4096.0
    # the same rows among more rows (dead ones) and a row's distance among other rows: the same bits
    x4 = torch.stack([x[0], torch.full((m,), float("nan")), torch.randn(m), x[1]])
    _, _, info4 = ops.centered_clip_reference(x4, 0b1001, 0.0, 1)
    assert info4["dist"][0].tolist() == [float(np.sqrt(tree)), 0.0, 0.0, float(np.sqrt(tree))]
    g = torch.Generator().manual_seed(3)
    m2 = 2 * 4096 + 4104  # three whole chunks and a ragged one
    rows = torch.randn(5, m2, generator=g) * torch.exp(3 * torch.randn(5, m2, generator=g))
    v = torch.randn(m2, generator=g)
    D5 = robust.cclip_distances(rows, v)
    for k in range(5):
        alone = robust.cclip_distances(rows[k:k + 1], v)
        want = tree_distance((rows[k] - v).numpy())
        assert float(D5[k]) == float(alone[0]) == float(want), k
    v[5] = float("inf")  # a coordinate whose centre is not finite never votes
    D = robust.cclip_distances(rows[:1], v)
    e = (rows[0] - v).numpy()
    e[5] = 0.0
    assert float(D[0]) == float(tree_distance(e))


# ------------------------------------------------------------------------------ what the rule buys
@pytest.mark.parametrize("kind", ATTACKS)
def test_closer_to_the_honest_mean_than_the_coordinate_wise_rules(kind):
    K, f = 8, 2
    for seed in range(5):
        x, hmean, att = attacked(honest_rows(seed, K), kind, f)
        res, w, _ = ops.centered_clip_reference(x, None, 0.0, 3)
        med = ops.trimmed_mean_reference(x, (K - 1) // 2)[0]
        trimmed = ops.trimmed_mean_reference(x, max(len(att), 1))[0]
        dc, dm, dt = rel_l2(res, hmean), rel_l2(med, hmean), rel_l2(trimmed, hmean)
        print(f"[cclip vs coordinate-wise] {kind} seed {seed}: cclip {dc:.4f} median {dm:.4f} trimmed {dt:.4f} "
              f"weights {[round(v, 3) for v in w.tolist()]}")
        assert dc < dm and dc < dt, (kind, seed, dc, dm, dt)
        honest = [float(w[k]) for k in range(K) if k not in att]
        assert all(float(w[k]) < min(honest) for k in att), (kind, seed, w)


# ------------------------------------------------------------------------------ real collectives
_N_COLL = 1003  # no multiple of 8 P: the exchange pads
_CASES = [(BF, 0.0, 3), (BF, 2.0, 1), (torch.float32, 0.0, 2)]


def _coll_input(rank: int, dtype) -> torch.Tensor:
    g = torch.Generator().manual_seed(177 + rank)
    x = torch.randn(_N_COLL, generator=g)
    x[::5] = 0.0
    if rank == 1:
        x[500:] = float("nan")  # bad in the later shards only
    return x.to(dtype)


def _coll_worker(rank, world, port, live):
    from distributedvolunteercomputing_amd.parallel.collectives import cclip_mean_
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    grp = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo")
    out = []
    for dtype, tau, iters in _CASES:
        t = _coll_input(rank, dtype)
        w = cclip_mean_(t, grp, tau, iters, live)
        out.append((bits(t).tolist(), w.tolist()))
    grp.barrier()
    return out


@pytest.mark.parametrize("P,live", [(2, None), (3, None), (4, None), (4, [0, 1, 3]), (3, [2, 0])])
def test_cclip_mean_over_gloo_matches_the_reference(P, live):
    from distributedvolunteercomputing_amd.parallel.collectives import _pad_len

    res = _mp.run(_coll_worker, P, live)
    mask = robust.mask_of(live, P)
    for i, (dtype, tau, iters) in enumerate(_CASES):
        L = _pad_len(_N_COLL, P, 8 if dtype == BF else 1)
        x = torch.zeros(P, L, dtype=dtype)
        for r in range(P):
            x[r, :_N_COLL] = _coll_input(r, dtype)
        m = L // P
        parts, ws = [], []
        for owner in range(P):  # every owner applies the rule to the peers' copies of its own shard
            r_, w_, _ = ops.centered_clip_reference(x[:, owner * m:(owner + 1) * m], mask, tau, iters)
            parts.append(r_)
            ws.append(w_.double())
        ref = torch.cat(parts)[:_N_COLL]
        wref = (sum(ws) / P).tolist()
        for r in range(P):
            got, w = res[r][i]
            assert got == bits(ref).tolist(), (dtype, tau, r)
            assert w == res[0][i][1], (dtype, tau, r)  # identical on every rank
            assert len(w) == P and all(abs(a - b) < 1e-6 for a, b in zip(w, wref)), (w, wref)
            assert all(w[k] == 0.0 for k in range(P) if not (mask >> k) & 1)


def test_cclip_mean_single_peer_is_the_identity():
    from distributedvolunteercomputing_amd.parallel.collectives import cclip_mean_

    t = _coll_input(1, BF)
    before = t.clone()
    w = cclip_mean_(t, None, 0.0, 3)
    assert torch.equal(bits(t), bits(before)) and w.tolist() == [1.0] and w.dtype == torch.float32
    for tau, iters in ((-1.0, 3), (float("nan"), 3), (0.0, 0), (0.0, 9)):
        with pytest.raises(ValueError):
            cclip_mean_(t, None, tau, iters)


def test_op_writes_every_row_and_refuses_bad_calls():
    P, n = 3, 40
    x, _ = family("normal", P, n)
    ref, wref, _ = ops.centered_clip_reference(x, None, 0.0, 2)
    inp = x.clone().view(-1)
    mine = torch.zeros(n, dtype=BF)
    w = torch.full((P,), 7.0)
    ops.cclip_reduce_bcast_bf16(inp, inp, mine, P, 0.0, 2, None, w)  # out aliases in
    assert torch.equal(bits(mine), bits(ref)) and torch.equal(w, wref)
    assert all(torch.equal(bits(inp.view(P, n)[k]), bits(ref)) for k in range(P))
    good = dict(P=3, tau=0.0, iters=2, mask=None)
    for bad in (dict(P=17), dict(mask=0), dict(mask=0b1000), dict(tau=-1.0), dict(tau=float("inf")),
                dict(tau=float("nan")), dict(iters=0), dict(iters=9), dict(iters=2.5)):
        kw = {**good, **bad}
        with pytest.raises(ValueError):
            ops.cclip_reduce_bcast_bf16(torch.zeros(kw["P"] * 8, dtype=BF), None, mine, kw["P"], kw["tau"],
                                        kw["iters"], kw["mask"])
    with pytest.raises(ValueError):
        ops.centered_clip_reference(torch.zeros(3, 8, dtype=torch.float16))
    assert "cclip" in robust.AGGREGATES and robust.AGGREGATES[:3] == ("mean", "trimmed", "median")


# ------------------------------------------------------------------------------ training
def _train_worker(rank, world, port, attack):
    from distributedvolunteercomputing_amd.jobs.train import BYZANTINE
    from distributedvolunteercomputing_amd.models.mlp import MLP, synthetic_mnist
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    g = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo")
    cfg = LocalSGDConfig(H=2, lr=0.05, weight_decay=0.0, max_grad_norm=0.0, comm_dtype=BF, aggregate="cclip")
    tr = LocalSGDTrainer(MLP(seed=0), cfg, group=g, device="cpu")
    if rank == world - 1:
        tr.delta_hook = BYZANTINE[attack]
    x, y = synthetic_mnist(512, seed=rank)
    losses, weights = [], []
    for i in range(12):
        b = slice((i % 8) * 64, (i % 8 + 1) * 64)
        out = tr.step(x[b], y[b])
        losses.append(float(out.extra["loss_t"]))
        if out.synced:
            weights.append(list(tr.clip_weight))
    g.barrier()
    return {"losses": losses, "anchor": hashlib.sha256(tr.anchor.numpy().tobytes()).hexdigest(),
            "finite": bool(torch.isfinite(tr.anchor).all()), "weights": weights, "syncs": tr.sync_count,
            "share": tr.trim_share}


@pytest.mark.parametrize("attack", ["nan", "flip", "scale"])
def test_training_survives_a_wrong_peer(attack):
    res = _mp.run(_train_worker, 4, attack)
    assert len({r["anchor"] for r in res.values()}) == 1
    print(f"[cclip {attack}] honest losses", [round(l, 4) for l in res[0]["losses"]], "weights", res[0]["weights"][-1])
    for rank, r in res.items():
        assert r["finite"] and r["syncs"] == 6 and r["share"] is None
        assert r["weights"] == res[0]["weights"] and len(r["weights"]) == 6
        for w in r["weights"]:
            assert len(w) == 4 and w[3] < min(w[:3]), w
            if attack == "nan":
                assert w[3] == 0.0
        if rank != 3:
            assert all(math.isfinite(l) for l in r["losses"]), r["losses"]
            assert r["losses"][-1] < r["losses"][0], r["losses"]


def _cli_worker(rank, world, port, metrics):
    from distributedvolunteercomputing_amd.jobs import train

    argv = ["--model", "mlp", "--steps", "12", "--H", "2", "--batch", "32", "--lr", "0.05", "--backend", "gloo",
            "--peer-id", str(rank), "--world", str(world), "--store-port", str(port), "--log-every", "2",
            "--aggregate", "cclip", "--clip-iters", "2", "--metrics", f"{metrics}.{rank}"]
    if rank == world - 1:
        argv += ["--byzantine", "scale"]
    return train.main(argv)


def test_train_cli_cclip_with_a_scaling_peer(tmp_path):
    base = str(tmp_path / "m.jsonl")
    res = _mp.run(_cli_worker, 4, base)
    assert all(v == 0 for v in res.values())
    recs = [json.loads(l) for l in open(base + ".0")]
    assert len(recs) == 6 and all(math.isfinite(r["loss"]) for r in recs)
    assert recs[-1]["loss"] < recs[0]["loss"]
    for r in recs:
        w = r["clip_weight"]
        assert len(w) == 4 and w[3] < min(w[:3]) and "trim_share" not in r, r


# ------------------------------------------------------------------------------ refusals, unchanged behaviour
def _lone_trainer(**kw):
    from distributedvolunteercomputing_amd.models.mlp import MLP
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer

    cfg = LocalSGDConfig(H=1, comm_dtype=BF, **kw)
    return LocalSGDTrainer(MLP(seed=0), cfg, device="cpu")


def test_refusals():
    from distributedvolunteercomputing_amd.jobs import train
    from distributedvolunteercomputing_amd.parallel.compression import (PowerSGDCompressor, Quant8Compressor,
                                                                        TopKCompressor)
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig

    for kw in (dict(clip_iters=0), dict(clip_iters=9), dict(clip_iters=2.0), dict(clip_tau=-0.5),
               dict(clip_tau=float("nan")), dict(clip_tau=float("inf"))):
        with pytest.raises(ValueError):
            LocalSGDConfig(aggregate="cclip", **kw)
    with pytest.raises(ValueError):
        LocalSGDConfig(aggregate="krum")
    cfg = LocalSGDConfig(aggregate="cclip")
    assert (cfg.clip_tau, cfg.clip_iters) == (0.0, 3) and LocalSGDConfig().aggregate == "mean"
    for make, name in ((lambda t: Quant8Compressor(t.flat.numel, "cpu"), "Quant8Compressor"),
                       (lambda t: TopKCompressor(t.flat.numel, 0.01, "cpu"), "TopKCompressor"),
                       (lambda t: PowerSGDCompressor(t.flat, 2, "cpu"), "PowerSGDCompressor")):
        tr = _lone_trainer(aggregate="cclip", robust_q8=True)
        tr.compressor = make(tr)
        with pytest.raises(ValueError, match=name):
            tr.sync()
    for algo in ("rccl", "rs_ag", "butterfly", "ring"):
        tr = _lone_trainer(aggregate="cclip", algo=algo)
        with pytest.raises(ValueError, match="direct"):
            tr.sync()
    tr = _lone_trainer(aggregate="cclip")
    tr.cfg.clip_iters = 9  # the config is mutable: the round checks again
    with pytest.raises(ValueError, match="iters"):
        tr.sync()
    tr = _lone_trainer(aggregate="cclip")
    tr.sync()  # alone: nothing to aggregate, nothing to refuse
    assert tr.clip_weight is None and _lone_trainer(aggregate="median").clip_weight is None
    for argv in (["--trainer", "sharded", "--aggregate", "cclip"], ["--aggregate", "cclip", "--clip-iters", "0"],
                 ["--aggregate", "cclip", "--clip-iters", "9"], ["--aggregate", "cclip", "--clip-tau", "-1"],
                 ["--aggregate", "cclip", "--clip-tau", "nan"], ["--aggregate", "cclip", "--clip-tau", "inf"],
                 ["--aggregate", "cclip", "--compression", "q8"], ["--aggregate", "cclip", "--compression", "topk"],
                 ["--aggregate", "cclip", "--compression", "powersgd"], ["--aggregate", "cclip", "--algo", "ring"],
                 ["--aggregate", "krum"]):
        with pytest.raises(SystemExit):
            train.parse(argv)
    a = train.parse(["--aggregate", "cclip", "--clip-tau", "0.5", "--clip-iters", "4", "--byzantine", "scale"])
    assert (a.aggregate, a.clip_tau, a.clip_iters, a.byzantine) == ("cclip", 0.5, 4, "scale")
    a = train.parse([])
    assert (a.aggregate, a.trim, a.clip_tau, a.clip_iters) == ("mean", 1, 0.0, 3)


def _buffers_worker(rank, world, port):
    from distributedvolunteercomputing_amd.parallel.flat_params import FlatBuffers
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    g = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo")
    bn = torch.nn.BatchNorm1d(4)
    bn.running_mean.fill_(float(rank))
    bn.running_var.fill_(float("nan") if rank == 2 else 1.0 + rank)
    fb = FlatBuffers(bn)
    out = {"median": fb.averaged(g, "median").tolist(), "cclip": fb.averaged(g, "cclip").tolist(),
           "median_live": fb.averaged(g, "median", 1, [0, 1, 3]).tolist(),
           "cclip_live": fb.averaged(g, "cclip", 5, [0, 1, 3]).tolist()}
    g.barrier()
    return out


def test_buffers_under_cclip_take_the_median_rule():
    res = _mp.run(_buffers_worker, 4)
    for r in res.values():
        assert r["cclip"] == r["median"] == [1.5] * 4 + [3.0] * 4
        assert r["cclip_live"] == r["median_live"]
