"""Trimmed-mean / median averaging on the torch reference: the rule itself, real gloo collectives,
local-SGD training next to a peer that sends wrong numbers, and the refusals."""
import hashlib
import json

import pytest
import torch

from distributedvolunteercomputing_amd import ops
from distributedvolunteercomputing_amd.ops import robust
from tests import _mp
from tests._robust import bits, family

BF = torch.bfloat16


def _row_order_mean(rows, dtype):
    """bf16/fp32 (sum in fp32, ascending row order, from +0) * fp32(1 / K)."""
    acc = torch.zeros(rows[0].numel(), dtype=torch.float32)
    for r in rows:
        acc = acc + r.float()
    inv = torch.tensor(1.0 / len(rows), dtype=torch.float32)
    return (acc * inv).to(dtype)


# ------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_key_order_is_float_order(dtype):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(16, 4096, generator=g) * torch.exp(8 * torch.randn(16, 4096, generator=g))).to(dtype)
    x[3, ::7] = 0.0
    x[5, ::7] = -0.0
    x[0, 0], x[1, 0] = float("inf"), -float("inf")
    order = torch.argsort(robust.order_keys(x), dim=0)
    v = x.double().gather(0, order)
    assert (v[1:] >= v[:-1]).all()
    # and the other way round: wherever the floats differ, the keys differ the same way
    k = robust.order_keys(x)
    lt = x.double()[:-1] < x.double()[1:]
    assert ((k[:-1] < k[1:]) == lt)[x.double()[:-1] != x.double()[1:]].all()


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_total_order_of_the_special_values(dtype):
    """-NaN < -Inf < -1 < -0 < +0 < 1 < +Inf < +NaN, whichever rows hold them; equal values go by row."""
    nan = torch.tensor([float("nan")], dtype=dtype)
    neg_nan = (bits(nan) | torch.iinfo(bits(nan).dtype).min).view(dtype)
    vals = torch.cat([nan, torch.tensor([0.0, float("inf"), -1.0, -0.0, -float("inf"), 1.0], dtype=dtype), neg_nan])
    k = robust.order_keys(vals.unsqueeze(1)).squeeze(1)
    assert torch.argsort(k).tolist() == [7, 5, 3, 4, 1, 6, 2, 0]
    z = torch.tensor([[0.0], [-0.0], [0.0]], dtype=dtype)
    assert torch.argsort(robust.order_keys(z).squeeze(1)).tolist() == [1, 0, 2]


@pytest.mark.parametrize("P,trim,mask", [(2, 1, 0b11), (3, 1, 0b111), (4, 1, 0b1111), (5, 2, 0b11111), (8, 3, 0xFF),
                                         (16, 7, 0xFFFF), (16, 2, 0xFFFF), (7, 1, 0b1011010), (9, 4, 0b110110111)])
def test_exactly_k_minus_2f_rows_are_kept_under_ties(P, trim, mask):
    g = torch.Generator().manual_seed(P)
    pool = torch.tensor([-0.0, 0.0, 1.0]).to(BF)
    x = pool[torch.randint(0, 3, (P, 2048), generator=g)]
    K, f, _ = robust.trim_plan(P, trim, mask)
    kept, live = robust.kept_rows(x, trim, mask)
    assert (kept.sum(0) == K - 2 * f).all()
    assert not kept[~live.squeeze(1)].any()
    _, counts = ops.trimmed_mean_reference(x, trim, mask)
    assert int(counts.sum()) == 2 * f * x.shape[1]


@pytest.mark.parametrize("P", [3, 4, 8])
def test_one_bad_row_is_trimmed_two_are_not(P):
    n = 4096
    x, mask = family("bad_row", P, n)
    bad = P // 2
    assert not torch.isfinite(x[bad].float()).all()
    res, counts = ops.trimmed_mean_reference(x, 1, mask)
    # 3e38 is finite: it is trimmed like the rest of that row, and the kept values are ordinary
    assert torch.isfinite(res.float()).all()
    assert int(counts[bad]) == n
    x[(bad + 1) % P] = float("nan")
    x[bad] = float("nan")
    res2, _ = ops.trimmed_mean_reference(x, 1, mask)
    assert not torch.isfinite(res2.float()).any()


@pytest.mark.parametrize("dtype,canon", [(BF, 0x7FC0), (torch.float32, 0x7FC00000)])
def test_a_nan_result_has_one_bit_pattern(dtype, canon):
    """NaN, -NaN and Inf - Inf all come out as the canonical quiet NaN, at every position of the vector
    (torch's own conversion to bf16 writes 0x7FC0 or 0xFFFF depending on the position)."""
    x, mask = family("bad_row", 3, 4104 + 5)
    x[0, ::2] = float("inf")  # meets -Inf in the bad row now and then
    res, _ = ops.trimmed_mean_reference(x.to(dtype), 0, mask)
    nan = torch.isnan(res)
    assert int(nan.sum()) > 1000 and bool(nan[-5:].any()) and bool(nan[:64].any())
    assert (bits(res)[nan].to(torch.int64) & (0xFFFF if dtype == BF else 0xFFFFFFFF) == canon).all()


@pytest.mark.parametrize("trim", [0, 1, 2])
def test_dead_rows_never_vote_and_are_never_counted(trim):
    P, n = 8, 1024
    x, mask = family("dead_rows", P, n)
    live = [k for k in range(P) if (mask >> k) & 1]
    assert len(live) == 4 and torch.isnan(x[1].float()).all()
    res, counts = ops.trimmed_mean_reference(x, trim, mask)
    ref, ref_counts = ops.trimmed_mean_reference(x[live], trim)
    assert torch.equal(bits(res), bits(ref)) and torch.isfinite(res.float()).all()
    assert counts[live].tolist() == ref_counts.tolist()
    assert all(int(counts[k]) == 0 for k in range(P) if k not in live)


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_trim_zero_is_the_row_order_mean(dtype):
    P, n = 5, 2048
    x, _ = family("normal", P, n)
    x = x.to(dtype)
    mask = 0b10111
    res, counts = ops.trimmed_mean_reference(x, 0, mask)
    assert torch.equal(bits(res), bits(_row_order_mean([x[k] for k in (0, 1, 2, 4)], dtype)))
    assert counts.tolist() == [0] * P


def test_one_and_two_voters_are_never_trimmed():
    x, _ = family("normal", 4, 512)
    for mask, rows in ((0b0100, [2]), (0b1001, [0, 3])):
        K, f, inv = robust.trim_plan(4, 3, mask)
        assert (K, f) == (len(rows), 0) and inv == 1.0 / K
        res, counts = ops.trimmed_mean_reference(x, 3, mask)
        assert torch.equal(bits(res), bits(_row_order_mean([x[k] for k in rows], BF)))
        assert counts.tolist() == [0, 0, 0, 0]
    assert robust.effective_trim("median", 1, 4) == 1 and robust.effective_trim("median", 1, 5) == 2
    even = torch.tensor([[1.0], [5.0], [2.0], [4.0]], dtype=BF)  # median of an even count: mean of the middle two
    assert float(ops.trimmed_mean_reference(even, robust.effective_trim("median", 0, 4))[0]) == 3.0


def test_op_writes_every_row_and_refuses_bad_calls():
    P, n = 3, 40
    x, _ = family("normal", P, n)
    ref, ref_counts = ops.trimmed_mean_reference(x, 1)
    inp = x.clone().view(-1)
    mine = torch.zeros(n, dtype=BF)
    counts = torch.ones(P, dtype=torch.int64)
    ops.trimmed_reduce_bcast_bf16(inp, inp, mine, P, 1, None, counts)  # out aliases in
    assert torch.equal(bits(mine), bits(ref)) and counts.tolist() == (ref_counts + 1).tolist()
    assert all(torch.equal(bits(inp.view(P, n)[k]), bits(ref)) for k in range(P))
    for bad in (dict(P=17, mask=None), dict(P=3, mask=0), dict(P=3, mask=0b1000)):
        with pytest.raises(ValueError):
            ops.trimmed_reduce_bcast_bf16(torch.zeros(bad["P"] * 8, dtype=BF), None, mine, bad["P"], 1, bad["mask"])
    with pytest.raises(ValueError):
        ops.trimmed_mean_reference(torch.zeros(3, 8, dtype=torch.float16), 1)


# ------------------------------------------------------------------------------ real collectives
_N_COLL = 1003  # no multiple of 8 P: the exchange pads, and the padding must not show in the counts
_CASES = [(BF, 0), (BF, 1), (BF, "median"), (torch.float32, 1)]


def _coll_input(rank: int, dtype) -> torch.Tensor:
    g = torch.Generator().manual_seed(77 + rank)
    x = torch.randn(_N_COLL, generator=g)
    x[::5] = 0.0  # ties across peers
    if rank == 1:
        x[::3] = float("nan")
    return x.to(dtype)


def _trim_of(trim, K):
    return robust.effective_trim("median", 0, K) if trim == "median" else trim


def _coll_worker(rank, world, port, live):
    from distributedvolunteercomputing_amd.parallel.collectives import robust_mean_
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    grp = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo")
    K = world if live is None else len(live)
    out = []
    for dtype, trim in _CASES:
        t = _coll_input(rank, dtype)
        counts = robust_mean_(t, grp, _trim_of(trim, K), live)
        out.append((bits(t).tolist(), counts.tolist()))
    grp.barrier()
    return out


@pytest.mark.parametrize("P,live", [(3, None), (4, None), (4, [0, 1, 3]), (3, [2, 0])])
def test_robust_mean_over_gloo_matches_the_reference(P, live):
    res = _mp.run(_coll_worker, P, live)
    mask = robust.mask_of(live, P)
    K = bin(mask).count("1")
    for i, (dtype, trim) in enumerate(_CASES):
        x = torch.stack([_coll_input(r, dtype) for r in range(P)])
        ref, ref_counts = ops.trimmed_mean_reference(x, _trim_of(trim, K), mask)
        for r in range(P):
            got, counts = res[r][i]
            assert got == bits(ref).tolist(), (dtype, trim, r)
            assert counts == ref_counts.tolist(), (dtype, trim, r)


def test_robust_mean_single_peer_is_the_identity():
    from distributedvolunteercomputing_amd.parallel.collectives import robust_mean_

    t = _coll_input(0, BF)
    before = t.clone()
    counts = robust_mean_(t, None, 1)
    assert torch.equal(bits(t), bits(before)) and counts.tolist() == [0]


# ------------------------------------------------------------------------------ training
def _attack(kind):
    from distributedvolunteercomputing_amd.jobs.train import BYZANTINE

    return BYZANTINE[kind]


def _train_worker(rank, world, port, aggregate, attack):
    from distributedvolunteercomputing_amd.models.mlp import MLP, synthetic_mnist
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    g = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo")
    cfg = LocalSGDConfig(H=2, lr=0.05, weight_decay=0.0, max_grad_norm=0.0, comm_dtype=BF, aggregate=aggregate, trim=1)
    tr = LocalSGDTrainer(MLP(seed=0), cfg, group=g, device="cpu")
    if rank == world - 1:
        tr.delta_hook = _attack(attack)
    x, y = synthetic_mnist(512, seed=rank)
    losses = []
    for i in range(12):
        b = slice((i % 8) * 64, (i % 8 + 1) * 64)
        losses.append(float(tr.step(x[b], y[b]).extra["loss_t"]))
    g.barrier()
    return {"losses": losses, "anchor": hashlib.sha256(tr.anchor.numpy().tobytes()).hexdigest(),
            "finite": bool(torch.isfinite(tr.anchor).all()), "share": tr.trim_share, "syncs": tr.sync_count}


def test_training_survives_a_nan_peer_with_the_trimmed_mean():
    res = _mp.run(_train_worker, 4, "trimmed", "nan")
    assert len({r["anchor"] for r in res.values()}) == 1
    for rank, r in res.items():
        assert r["finite"] and r["syncs"] == 6
        assert r["share"][3] == 1.0 and all(s < 0.75 for s in r["share"][:3]), r["share"]
        if rank != 3:
            assert all(l == l and abs(l) != float("inf") for l in r["losses"]), r["losses"]
            assert r["losses"][-1] < r["losses"][0], r["losses"]
    print("[robust nan] honest losses", [round(l, 4) for l in res[0]["losses"]], "shares", res[0]["share"])


def test_training_with_the_plain_mean_is_poisoned_by_the_same_peer():
    """The control: the same run under aggregate="mean" ends with a non-finite anchor on every peer."""
    res = _mp.run(_train_worker, 4, "mean", "nan")
    for r in res.values():
        assert not r["finite"] and r["share"] is None


def test_training_survives_a_sign_flipping_peer():
    res = _mp.run(_train_worker, 4, "trimmed", "flip")
    assert len({r["anchor"] for r in res.values()}) == 1
    for rank, r in res.items():
        assert r["finite"]
        if rank != 3:
            assert r["losses"][-1] < r["losses"][0], r["losses"]


# ------------------------------------------------------------------------------ refusals and the CLI
def _lone_trainer(**kw):
    from distributedvolunteercomputing_amd.models.mlp import MLP
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer

    cfg = LocalSGDConfig(H=1, comm_dtype=BF, **kw)
    return LocalSGDTrainer(MLP(seed=0), cfg, device="cpu")


def test_refusals():
    from distributedvolunteercomputing_amd.jobs import train
    from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig

    for kw in (dict(aggregate="krum"), dict(aggregate="trimmed", trim=-1), dict(aggregate="trimmed", trim=1.5)):
        with pytest.raises(ValueError):
            LocalSGDConfig(**kw)
    tr = _lone_trainer(aggregate="median")
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    with pytest.raises(ValueError, match="compressor"):
        tr.sync()
    tr = _lone_trainer(aggregate="trimmed", algo="rccl")
    with pytest.raises(ValueError, match="direct"):
        tr.sync()
    tr = _lone_trainer(aggregate="trimmed")
    tr.cfg.aggregate = "krum"  # the config is mutable: the round checks again
    with pytest.raises(ValueError):
        tr.sync()
    _lone_trainer(aggregate="trimmed").sync()  # alone: nothing to aggregate, nothing to refuse
    for argv in (["--trainer", "sharded", "--aggregate", "median"], ["--trainer", "sharded", "--byzantine", "nan"],
                 ["--aggregate", "krum"], ["--byzantine", "loud"], ["--aggregate", "trimmed", "--trim", "-1"]):
        with pytest.raises(SystemExit):
            train.parse(argv)
    a = train.parse(["--aggregate", "trimmed", "--trim", "2", "--byzantine", "scale"])
    assert (a.aggregate, a.trim, a.byzantine) == ("trimmed", 2, "scale")
    a = train.parse([])
    assert (a.aggregate, a.trim, a.byzantine) == ("mean", 1, "none")


def test_newcomers_do_not_vote():
    """Voters are positions in the generation's member list; with nobody but newcomers everyone votes."""
    from types import SimpleNamespace

    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDTrainer

    g = SimpleNamespace(members=[5, 7, 9])
    assert LocalSGDTrainer._voters(g, ()) is None
    assert LocalSGDTrainer._voters(g, {7}) == [0, 2]
    assert LocalSGDTrainer._voters(g, {5, 7, 9}) is None


def test_flat_buffers_robust_average_defaults_to_the_mean():
    """averaged(group) keeps today's arithmetic; with one peer there is nothing to average either way."""
    from distributedvolunteercomputing_amd.parallel.flat_params import FlatBuffers

    bn = torch.nn.BatchNorm1d(4)
    fb = FlatBuffers(bn)
    assert fb.averaged(None) is None and fb.averaged(None, "median") is None


def _buffers_worker(rank, world, port):
    from distributedvolunteercomputing_amd.parallel.flat_params import FlatBuffers
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    g = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo")
    bn = torch.nn.BatchNorm1d(4)
    bn.running_mean.fill_(float(rank))
    bn.running_var.fill_(float("nan") if rank == 2 else 1.0 + rank)
    fb = FlatBuffers(bn)
    out = {"mean": fb.averaged(g).tolist(), "median": fb.averaged(g, "median").tolist(),
           "trimmed": fb.averaged(g, "trimmed", 1, [0, 1, 2]).tolist()}
    g.barrier()
    return out


def test_flat_buffers_robust_average_over_gloo():
    res = _mp.run(_buffers_worker, 4)
    for r in res.values():
        assert r["mean"][:4] == [1.5] * 4 and r["mean"][4] != r["mean"][4]  # the mean takes the NaN in
        assert r["median"] == [1.5] * 4 + [3.0] * 4  # mean of the middle two of {0,1,2,3} and of {1,2,4,NaN}
        assert r["trimmed"] == [1.0] * 4 + [2.0] * 4  # voters 0..2, one trimmed at each end


def _cli_worker(rank, world, port, metrics):
    from distributedvolunteercomputing_amd.jobs import train

    argv = ["--model", "mlp", "--steps", "12", "--H", "2", "--batch", "32", "--lr", "0.05", "--backend", "gloo",
            "--peer-id", str(rank), "--world", str(world), "--store-port", str(port), "--log-every", "2",
            "--aggregate", "trimmed", "--trim", "1", "--metrics", f"{metrics}.{rank}"]
    if rank == world - 1:
        argv += ["--byzantine", "nan"]
    return train.main(argv)


def test_train_cli_trimmed_with_a_nan_peer(tmp_path):
    base = str(tmp_path / "m.jsonl")
    res = _mp.run(_cli_worker, 4, base)
    assert all(v == 0 for v in res.values())
    recs = [json.loads(l) for l in open(base + ".0")]
    assert len(recs) == 6 and all(r["loss"] == r["loss"] for r in recs)
    assert recs[-1]["loss"] < recs[0]["loss"]
    assert all(r["trim_share"][3] == 1.0 and len(r["trim_share"]) == 4 for r in recs)
