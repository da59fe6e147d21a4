"""Trimmed-mean / median averaging over the q8 exchange, on the torch definition: the rule on 8-bit
records, real gloo collectives, local-SGD training next to a peer that sends NaN scales, the refusals
and the train CLI."""
import hashlib
import json

import pytest
import torch

from distributedvolunteercomputing_amd.ops import robust
from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor, q8_quantise
from tests import _mp
from tests._q8_robust import BLOCK, codes_of, decoded, family, pack, run_reduce_robust, scales_of, set_scales

BF = torch.bfloat16


def _record_of(res: torch.Tensor) -> torch.Tensor:
    return pack(*q8_quantise(res.view(-1, BLOCK)))


# ------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("P", [2, 3, 5, 8, 16])
def test_trim_zero_is_reduce_byte_for_byte(P):
    """All rows live, honest records, valid = m: the plain mean is the special case."""
    bps = 5
    rec, mask = family("honest", P, bps)
    comp = Quant8Compressor(P * bps * BLOCK, "cpu")
    want = comp.reduce(rec.reshape(-1), P).clone()
    got, counts, nonfinite = run_reduce_robust(rec, 0, mask, bps * BLOCK)
    assert torch.equal(got, want) and counts == [0] * P and nonfinite == 0


def _garbage(P, bps, rows, seed):
    rec, mask = family("garbage_row", P, bps, seed)
    bad = P // 2
    for k in rows:  # further garbage rows: the same bytes, rotated
        rec[k] = torch.roll(rec[bad], 4 * k)
    return rec, mask, sorted({bad, *rows})


@pytest.mark.parametrize("P,f,extra", [(3, 1, ()), (5, 1, ()), (5, 2, (0,)), (8, 3, (1, 6)), (16, 2, (15,)),
                                       (16, 7, ())])
def test_the_guarantee_holds_with_up_to_f_garbage_rows(P, f, extra):
    """With at most f rows of arbitrary bytes every result is finite and lies within the honest rows' decoded
    range. The range is widened for the fp32 arithmetic: n = K - 2f kept values of magnitude at most A, summed in
    fp32 (n - 1 additions, each off by at most 2^-24 of a partial sum that is at most n A), then one multiply by
    an inv that is itself rounded: (n - 1) + 2 = n + 1 units of 2^-24 A, plus 2^-149 for a product that lands among
    the subnormals.
    The garbage row is trimmed at 90% of the elements at least: asserted under the median (f = (K - 1) // 2), where
    a garbage value is kept only if it is itself the middle of the column. Under a smaller f it is also kept wherever
    f honest values lie on either side of it, which is what the rule promises and no fault: with honest values of
    randn * exp(4 randn) and K - 1 - 2f spare honest rows that is no rare event (the shares printed below: 0.85 to
    0.88 at P = 5, f = 1 and 0.74 to 0.85 for the two garbage rows at P = 16, f = 2), so no share is asserted there."""
    bps = 9  # every planted scale at least once
    m = bps * BLOCK
    for seed in (0, 3):
        rec, mask, bad = _garbage(P, bps, extra, seed)
        assert len(bad) <= f
        planted = scales_of(rec)[P // 2]
        assert torch.isnan(planted).any() and torch.isinf(planted).any() and (planted == 0).any()
        assert (codes_of(rec)[P // 2] == -128).any()
        for valid in (m, m - 5):
            dec = decoded(rec)[:, :valid]
            res, counts = robust.trimmed_mean_reference(torch.where(torch.isnan(dec), torch.full_like(dec, float("nan")),
                                                                    dec), f, mask)
            good = [k for k in range(P) if k not in bad]
            lo, hi = dec[good].min(0).values, dec[good].max(0).values
            A = torch.maximum(lo.abs(), hi.abs()).double()
            w = (P - 2 * f + 1) * 2.0 ** -24 * A + 2.0 ** -149
            assert torch.isfinite(res).all()
            assert (res.double() >= lo.double() - w).all() and (res.double() <= hi.double() + w).all()
            got, c, nonfinite = run_reduce_robust(rec, f, mask, valid)
            assert nonfinite == 0 and c == counts.tolist()
            print(f"[q8 robust guarantee] P={P} f={f} seed={seed} valid={valid}: garbage rows trimmed at",
                  [round(c[k] / valid, 4) for k in bad])
            if f == (P - 1) // 2:
                assert c[P // 2] >= 0.9 * valid, c
            full = torch.zeros(m)
            full[:valid] = res
            assert torch.equal(got, _record_of(full))  # the record is the codec's record of exactly these results
            assert torch.isfinite(scales_of(got.unsqueeze(0))).all()


@pytest.mark.parametrize("P,f", [(3, 1), (5, 1), (8, 2)])
def test_over_budget_coordinates_come_out_as_zero_and_are_counted(P, f):
    bps = 3
    m = bps * BLOCK
    rec, mask = family("over_budget", P, bps, f=f)
    valid = m - 5
    got, counts, nonfinite = run_reduce_robust(rec, f, mask, valid)
    # f + 1 rows are NaN at every coordinate: f are trimmed from the top, one is kept, the sum is NaN
    assert nonfinite == valid
    assert not got.any()  # zero codes, zero scales: no update, and nothing non-finite on the wire
    # one NaN block only: the other blocks keep their values, and every scale stays finite
    rec2, _ = family("honest", P, bps)
    for k in range(f + 1):
        sc = scales_of(rec2)[k].view(torch.int32).tolist()
        set_scales(rec2, k, [0x7FC00000] + [x & 0xFFFFFFFF for x in sc[1:]])
    got2, _, nonfinite2 = run_reduce_robust(rec2, f, mask, m)
    assert nonfinite2 == BLOCK
    s2 = scales_of(got2.unsqueeze(0))[0]
    assert torch.isfinite(s2).all() and float(s2[0]) == 0.0 and (s2[1:] > 0).all()
    assert not codes_of(got2.unsqueeze(0))[0, :BLOCK].any()


@pytest.mark.parametrize("P", [3, 8])
def test_padding_does_not_vote(P):
    bps = 2
    m = bps * BLOCK
    rec, mask = family("honest", P, bps)
    valid = m - 37
    want = run_reduce_robust(rec, 1, mask, valid)
    dirty = rec.clone()
    g = torch.Generator().manual_seed(9)
    codes_of(dirty)[:, valid:] = torch.randint(-128, 128, (P, m - valid), generator=g, dtype=torch.int8)
    got = run_reduce_robust(dirty, 1, mask, valid)
    assert torch.equal(got[0], want[0]) and got[1:] == want[1:]
    assert sum(want[1]) == 2 * valid  # f = 1: two rows trimmed at every element that votes, none beyond
    assert not codes_of(want[0].unsqueeze(0))[0, valid:].any()
    # the last real block's scale comes from the real elements alone
    clean = decoded(rec)[:, :valid]
    res, _ = robust.trimmed_mean_reference(clean, 1, mask)
    assert float(scales_of(want[0].unsqueeze(0))[0, -1]) == float(q8_quantise(
        torch.cat([res, torch.zeros(m - valid)]).view(-1, BLOCK))[1][-1])
    empty = run_reduce_robust(dirty, 1, mask, 0)
    assert not empty[0].any() and empty[1] == [0] * P and empty[2] == 0


def test_dead_rows_and_newcomers_do_not_vote():
    P, bps = 5, 3
    m = bps * BLOCK
    rec, mask = family("dead_rows", P, bps)
    live = [k for k in range(P) if (mask >> k) & 1]
    got = run_reduce_robust(rec, 1, mask, m)
    want = run_reduce_robust(rec[live].contiguous(), 1, (1 << len(live)) - 1, m)
    assert torch.equal(got[0], want[0]) and [got[1][k] for k in live] == want[1] and got[2] == 0
    assert all(got[1][k] == 0 for k in range(P) if k not in live)
    # a newcomer's all-zero record: it would pull every coordinate towards 0 if it voted
    rec, _ = family("honest", P, bps)
    rec[4] = 0
    voters = robust.mask_of([0, 1, 2, 3], P)
    got = run_reduce_robust(rec, 1, voters, m)
    want = run_reduce_robust(rec[:4].contiguous(), 1, 0b1111, m)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] + [0]
    assert not torch.equal(run_reduce_robust(rec, 1, (1 << P) - 1, m)[0], got[0])


def test_reduce_robust_refuses_bad_calls():
    P, bps = 3, 2
    m = bps * BLOCK
    rec, mask = family("honest", P, bps)
    comp = Quant8Compressor(P * m, "cpu")
    flat = rec.reshape(-1)
    for kw in (dict(live_mask=0), dict(live_mask=0b1000), dict(valid=-1), dict(valid=m + 1), dict(trim=-1),
               dict(recv=flat[:-4]), dict(counts=torch.zeros(P, dtype=torch.int32)),
               dict(counts=torch.zeros(P - 1, dtype=torch.int64)), dict(nonfinite=torch.zeros(2, dtype=torch.int64))):
        args = dict(recv=flat, P=P, trim=1, live_mask=mask, valid=m)
        args.update(kw)
        with pytest.raises(ValueError):
            comp.reduce_robust(**args)
    with pytest.raises(ValueError):
        Quant8Compressor(17 * m, "cpu").reduce_robust(torch.zeros(17 * (m + m // 32), dtype=torch.uint8), 17, 1, None, m)
    comp.reduce_robust(flat, P, 1, None, m)  # and the same call with nothing wrong goes through


# ------------------------------------------------------------------------------ real collectives
_N_COLL = 128 * 7 + 45  # no multiple of 128 P: the last shards are padded, and the padding must not show


def _coll_input(rank: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(31 + rank)
    x = torch.randn(_N_COLL, generator=g) * torch.exp(torch.randn(_N_COLL, generator=g))
    x[::5] = 0.0
    return x.to(BF)


def _nan_scales():
    from distributedvolunteercomputing_amd.jobs.train import nan_scales

    return nan_scales


def _coll_worker(rank, world, port, live, trim):
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    grp = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo")
    comp = Quant8Compressor(_N_COLL, "cpu")
    if rank == 1:
        comp.wire_hook = _nan_scales()
    out = []
    for _ in range(2):  # the second round carries the error feedback of the first
        avg, counts, nonfinite = comp.allreduce_robust(_coll_input(rank), grp, trim, live)
        out.append((avg.view(torch.int16).tolist(), counts.tolist(), nonfinite))
    grp.barrier()
    return out, comp.e.tolist(), comp.bytes_sent


def _simulate(P, live, trim, rounds=2):
    """The same rounds in one process: encode on every peer, shuffle the records by hand, reduce_robust on every
    shard owner, decode the concatenated records."""
    comps = [Quant8Compressor(_N_COLL, "cpu") for _ in range(P)]
    comps[1].wire_hook = _nan_scales()
    mask = robust.mask_of(live, P)
    L, m, rec = comps[0].layout(P)
    out = []
    for _ in range(rounds):
        wires = [comps[r].encode(_coll_input(r), P).view(P, rec).clone() for r in range(P)]
        records, counts, nonfinite = [], torch.zeros(P, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
        for j in range(P):
            recv = torch.stack([wires[r][j] for r in range(P)]).reshape(-1)
            valid = min(max(_N_COLL - j * m, 0), m)
            records.append(comps[j].reduce_robust(recv, P, trim, mask, valid, counts, nonfinite).clone())
        avg = comps[0].decode(torch.cat(records), P)
        out.append((avg.view(torch.int16).tolist(), counts.tolist(), int(nonfinite)))
    return out, [c.e.tolist() for c in comps]


@pytest.mark.parametrize("P,live,trim", [(3, None, 1), (5, None, 1), (5, [0, 1, 2, 4], 2)])
def test_allreduce_robust_over_gloo_is_the_one_process_simulation(P, live, trim):
    res = _mp.run(_coll_worker, P, live, trim)
    want, want_e = _simulate(P, live, trim)
    L, m, rec = Quant8Compressor(_N_COLL, "cpu").layout(P)
    for r in range(P):
        rounds, e, sent = res[r]
        assert rounds == want, r  # the average and both counters, identical on every rank
        assert e == want_e[r], r
        assert sent == 2 * (2 * (P - 1) * rec + 8 * (P + 1))
    K = P if live is None else len(live)
    f = min(trim, (K - 1) // 2)
    for avg, counts, nonfinite in want:
        assert counts[1] == _N_COLL and nonfinite == 0 and sum(counts) == 2 * f * _N_COLL
        assert torch.isfinite(torch.tensor(avg, dtype=torch.int16).view(BF).float()).all()


def test_allreduce_robust_alone_is_one_record_of_the_own_values():
    comp, ref = Quant8Compressor(_N_COLL, "cpu"), Quant8Compressor(_N_COLL, "cpu")
    avg, counts, nonfinite = comp.allreduce_robust(_coll_input(0), None, 1)
    # K = 1: nothing is trimmed, and quantising the decoded record again gives the same record
    assert torch.equal(avg.view(torch.int16), ref.allreduce_mean(_coll_input(0), None).view(torch.int16))
    assert counts.tolist() == [0] and nonfinite == 0


# ------------------------------------------------------------------------------ training
def _train_worker(rank, world, port, aggregate):
    from distributedvolunteercomputing_amd.models.mlp import MLP, synthetic_mnist
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    g = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo")
    cfg = LocalSGDConfig(H=2, lr=0.05, weight_decay=0.0, max_grad_norm=0.0, comm_dtype=BF, aggregate=aggregate, trim=1,
                         robust_q8=True)
    tr = LocalSGDTrainer(MLP(seed=0), cfg, group=g, device="cpu")
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    if rank == world - 1:
        tr.wire_hook = _nan_scales()
    x, y = synthetic_mnist(512, seed=rank)
    start = tr.anchor.clone()
    losses = []
    for i in range(12):
        b = slice((i % 8) * 64, (i % 8 + 1) * 64)
        losses.append(float(tr.step(x[b], y[b]).extra["loss_t"]))
    g.barrier()
    return {"losses": losses, "anchor": hashlib.sha256(tr.anchor.numpy().tobytes()).hexdigest(),
            "finite": bool(torch.isfinite(tr.anchor).all()), "share": tr.trim_share, "syncs": tr.sync_count,
            "nonfinite": tr.nonfinite_share, "ef_finite": bool(torch.isfinite(tr.compressor.e).all()),
            "moved": not torch.equal(tr.anchor, start)}


def test_training_over_q8_survives_a_nan_peer_with_the_trimmed_mean():
    """The criterion of tests/test_robust_cpu.py for the uncompressed pair, with q8 in between."""
    res = _mp.run(_train_worker, 4, "trimmed")
    assert len({r["anchor"] for r in res.values()}) == 1
    for rank, r in res.items():
        assert r["finite"] and r["moved"] and r["syncs"] == 6 and r["nonfinite"] == 0.0 and r["ef_finite"]
        assert r["share"][3] == 1.0 and all(s < 0.75 for s in r["share"][:3]), r["share"]
        if rank != 3:
            assert all(l == l and abs(l) != float("inf") for l in r["losses"]), r["losses"]
            assert r["losses"][-1] < r["losses"][0], r["losses"]
    print("[q8 robust nan] honest losses", [round(l, 4) for l in res[0]["losses"]], "shares", res[0]["share"])


def test_training_over_q8_with_the_plain_mean_is_poisoned_by_the_same_peer():
    """The control: under aggregate="mean" one peer's NaN scales reach every block of every sum. What comes out of
    a NaN sum is not defined by the codec; the torch codec sends such a block as nothing (scale 0), so the six rounds
    deliver no update at all and the model the peers share is still the initial one (a codec that let the NaN through
    would leave a non-finite model instead). Either way the peers' training is lost."""
    res = _mp.run(_train_worker, 4, "mean")
    for r in res.values():
        assert (not r["finite"]) or (not r["moved"]), r
        assert r["share"] is None and r["nonfinite"] is None


# ------------------------------------------------------------------------------ refusals and the CLI
def _lone_trainer(**kw):
    from distributedvolunteercomputing_amd.models.mlp import MLP
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer

    cfg = LocalSGDConfig(H=1, comm_dtype=BF, **kw)
    return LocalSGDTrainer(MLP(seed=0), cfg, device="cpu")


def test_refusals():
    from distributedvolunteercomputing_amd.jobs import train
    from distributedvolunteercomputing_amd.parallel.compression import PowerSGDCompressor, TopKCompressor

    for make in (lambda t: TopKCompressor(t.flat.numel, 0.01, "cpu"), lambda t: PowerSGDCompressor(t.flat, 2, "cpu")):
        for asked in (False, True):  # asking for q8 does not make another compressor legal
            tr = _lone_trainer(aggregate="median", robust_q8=asked)
            tr.compressor = make(tr)
            with pytest.raises(ValueError, match="q8 is the compressor that works"):
                tr.sync()
    tr = _lone_trainer(aggregate="trimmed")
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    with pytest.raises(ValueError, match="robust_q8"):  # not asked for: refused as before, and the message says how
        tr.sync()
    tr = _lone_trainer(aggregate="trimmed", robust_q8=True)
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    tr.sync()  # q8 is accepted (alone: nothing to aggregate)
    tr = _lone_trainer(aggregate="mean")
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    tr.sync()  # the plain mean never needed the request
    tr = _lone_trainer(aggregate="trimmed", algo="rccl", robust_q8=True)
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    with pytest.raises(ValueError, match="direct"):
        tr.sync()
    for argv in (["--trainer", "sharded", "--aggregate", "median", "--compression", "q8"],
                 ["--trainer", "sharded", "--byzantine", "nan", "--compression", "q8"]):
        with pytest.raises(SystemExit):
            train.parse(argv)
    a = train.parse(["--aggregate", "trimmed", "--compression", "q8", "--byzantine", "nan"])
    assert (a.aggregate, a.compression, a.byzantine) == ("trimmed", "q8", "nan")


def _cli_worker(rank, world, port, metrics):
    from distributedvolunteercomputing_amd.jobs import train

    argv = ["--model", "mlp", "--steps", "12", "--H", "2", "--batch", "32", "--lr", "0.05", "--backend", "gloo",
            "--peer-id", str(rank), "--world", str(world), "--store-port", str(port), "--log-every", "2",
            "--aggregate", "trimmed", "--trim", "1", "--compression", "q8", "--metrics", f"{metrics}.{rank}"]
    if rank == world - 1:
        argv += ["--byzantine", "nan"]
    return train.main(argv)


def test_train_cli_q8_trimmed_with_a_nan_peer(tmp_path):
    base = str(tmp_path / "m.jsonl")
    res = _mp.run(_cli_worker, 4, base)
    assert all(v == 0 for v in res.values())
    recs = [json.loads(l) for l in open(base + ".0")]
    assert len(recs) == 6 and all(r["loss"] == r["loss"] for r in recs)
    assert recs[-1]["loss"] < recs[0]["loss"]
    assert all(r["trim_share"][3] >= 0.99 and len(r["trim_share"]) == 4 for r in recs)
    assert all(r["nonfinite_share"] == 0 for r in recs)
