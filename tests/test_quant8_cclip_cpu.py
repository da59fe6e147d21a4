"""Centered clipping over the q8 records on the CPU: the torch definition (Quant8Compressor.reduce_cclip_reference)
against an independent recomputation, its edge shapes, the bounds the rule promises, what it buys against the median,
the trainer's and the CLI's switches, a real gloo round and an aborted one."""
import hashlib
import json
import math
import struct

import numpy as np
import pytest
import torch

from distributedvolunteercomputing_amd.ops import robust
from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor, q8_quantise
from tests import _mp
from tests._cclip import ATTACKS, attacked, honest_rows, rel_l2, tree_distance
from tests._q8_cclip import FAMILIES, NAN, bad_blocks, clipping_tau, family, reference, run_reduce_cclip
from tests._q8_robust import BLOCK, PLANTED, decoded, pack, scales_of, set_scales

BF = torch.bfloat16


def _fp32(a: float) -> float:
    return struct.unpack("f", struct.pack("f", a))[0]


def _canonical_decoded(rec: torch.Tensor) -> torch.Tensor:
    dec = decoded(rec)
    nan = torch.tensor([NAN], dtype=torch.int32).view(torch.float32)
    return torch.where(torch.isnan(dec), nan, dec)


def _independent(rec, mask, valid, tau, iters):
    """(record, weights list, nonfinite) of the rule, recomputed with numpy fp32 vectors, tests/_cclip.tree_distance
    for the distances and Python floats for the square root and the divide. Only the median start comes from
    ops/robust.py (tests/test_robust_cpu.py holds that rule to its own oracle)."""
    P = rec.shape[0]
    m = rec.shape[1] * 32 // 33
    dec = _canonical_decoded(rec)[:, :valid]
    rows = [k for k in range(P) if (mask >> k) & 1]
    K = len(rows)
    w = [0.0] * P
    if K == 1:
        res = dec[rows[0]].numpy().copy()
        w[rows[0]] = 1.0
    else:
        v = robust.trimmed_mean_reference(dec, (K - 1) // 2, mask)[0].numpy().copy()
        x = dec[rows].numpy()
        inv_k = np.float32(1.0 / K)
        with np.errstate(all="ignore"):
            for _ in range(iters):
                fin = np.isfinite(v)
                D = [float(tree_distance(np.where(fin, x[i] - v, np.float32(0.0)))) for i in range(K)]
                d = [_fp32(math.sqrt(a)) if math.isfinite(a) else math.inf for a in D]
                t = _fp32(tau) if tau > 0 else sorted(d)[(K - 1) // 2]
                wl = [0.0 if a == math.inf else (1.0 if a <= t else _fp32(t / a)) for a in d]
                acc = np.zeros_like(v)
                for i in range(K):
                    if wl[i] > 0:
                        acc = acc + np.float32(wl[i]) * (x[i] - v)
                v = np.where(fin, v + acc * inv_k, v).astype(np.float32)
            for i, k in enumerate(rows):
                w[k] = wl[i]
        res = v
    res = torch.from_numpy(res)
    bad = ~torch.isfinite(res)
    out = torch.zeros(m)
    out[:valid] = torch.where(bad, torch.zeros_like(res), res)
    return pack(*q8_quantise(out.view(-1, BLOCK))), w, int(bad.sum())


def _w_bits(w):
    return torch.as_tensor(w, dtype=torch.float32).view(torch.int32).tolist()


# ------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("name", FAMILIES)
def test_the_reference_is_the_composition(name, P):
    bps = 33
    m = bps * BLOCK
    rec, mask = family(name, P, bps)
    for tau in (0.0, clipping_tau(rec, mask, m)):
        for iters in (1, 3):
            for valid in (m, m - 77):
                got, w, bad, info = reference(rec, mask, valid, tau, iters)
                want, ww, wbad = _independent(rec, mask, valid, tau, iters)
                tag = (name, P, tau, iters, valid)
                assert torch.equal(got, want), tag
                assert _w_bits(w) == _w_bits(ww) and int(bad) == wbad, (tag, w.tolist(), ww, int(bad), wbad)
                assert info["result"].shape == (valid,) and len(info["centres"]) == iters + 1
                # the method on CPU tensors is the reference
                mrec, mw, mbad = run_reduce_cclip(rec, mask, valid, tau, iters)
                assert torch.equal(mrec, got) and _w_bits(mw) == _w_bits(w) and mbad == int(bad), tag
    if name == "majority_bad":
        frozen = len(bad_blocks(bps)) * BLOCK
        got, w, bad, info = reference(rec, mask, m, 0.0, 3)
        assert int(bad) == frozen  # the frozen coordinates, all counted, all sent as zero
        assert torch.isnan(info["result"]).sum() == frozen
    if name == "far_row":
        w = reference(rec, mask, m, 0.0, 3)[1]
        assert 0.0 < float(w[P - 1]) < 1.0, w.tolist()


@pytest.mark.parametrize("P", [2, 3, 5, 8, 16])
def test_shapes(P):
    bps = 33
    m = bps * BLOCK
    for name in ("honest", "garbage_row", "majority_bad"):
        rec, mask = family(name, P, bps)
        if name == "garbage_row":
            assert set(PLANTED) <= {x & 0xFFFFFFFF for x in scales_of(rec)[P // 2].view(torch.int32).tolist()}
        for valid in (m, m - 77, 128, 0):
            got, w, bad, info = reference(rec, mask, valid, 0.0, 2)
            dec = decoded(got.unsqueeze(0))[0]
            assert torch.isfinite(dec).all() and not dec[valid:].any(), (name, valid)
            assert int(bad) == int((~torch.isfinite(info["result"])).sum())
            if valid == 0:
                assert not got.any() and int(bad) == 0 and w.tolist() == [1.0] * P
    # one voter: its decoded row through the finish, whatever it holds; weight 1 for it alone
    rec, _ = family("garbage_row", P, bps)
    row = P // 2
    got, w, bad, info = reference(rec, 1 << row, m - 77, 0.0, 3)
    dec = _canonical_decoded(rec)[row, :m - 77]
    fin = torch.isfinite(dec)
    want = torch.zeros(m)
    want[:m - 77] = torch.where(fin, dec, torch.zeros_like(dec))
    assert torch.equal(got, pack(*q8_quantise(want.view(-1, BLOCK))))
    assert int(bad) == int((~fin).sum()) > 0 and w.tolist() == [1.0 if k == row else 0.0 for k in range(P)]


@pytest.mark.parametrize("P", [3, 8])
def test_dead_rows_are_never_read(P):
    bps = 33
    m = bps * BLOCK
    rec, mask = family("dead_rows", P, bps)  # the dead rows hold 0xFF
    other = rec.clone()
    for k in range(P):
        if not (mask >> k) & 1:
            other[k] = family("honest", P, bps, seed=3)[0][k]
            set_scales(other, k, [NAN] * bps)
    for tau in (0.0, clipping_tau(rec, mask, m)):
        a = reference(rec, mask, m - 77, tau, 3)
        b = reference(other, mask, m - 77, tau, 3)
        assert torch.equal(a[0], b[0]) and _w_bits(a[1]) == _w_bits(b[1]) and int(a[2]) == int(b[2])
        assert all(float(a[1][k]) == 0.0 for k in range(P) if not (mask >> k) & 1)


def test_reduce_cclip_refuses_bad_calls():
    P, bps = 3, 2
    m = bps * BLOCK
    comp = Quant8Compressor(P * m, "cpu")
    good = torch.zeros(P * (m + m // 32), dtype=torch.uint8)
    ok = dict(recv=good, P=P, live_mask=0b111, valid=m, tau=0.0, iters=3)
    for kw in (dict(live_mask=0), dict(live_mask=0b1000), dict(valid=m + 1), dict(valid=-1), dict(recv=good[:-4]),
               dict(recv=good.view(torch.int8)), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")),
               dict(tau=1e39), dict(iters=0), dict(iters=9), dict(weights=torch.zeros(P, dtype=torch.float64)),
               dict(weights=torch.zeros(P + 1)), dict(nonfinite=torch.zeros(1, dtype=torch.int32)),
               dict(nonfinite=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            comp.reduce_cclip(**dict(ok, **kw))
    assert not comp.reduce_cclip(**ok).any()
    e0 = comp.e.clone()
    for kw in (dict(tau=-1.0), dict(iters=9), dict(live_ranks=[3])):  # every refusal before e is touched
        with pytest.raises(ValueError):
            comp.allreduce_cclip(torch.ones(P * m, dtype=BF), None, **dict(dict(tau=0.0, iters=3), **kw))
        assert torch.equal(comp.e, e0)


# ------------------------------------------------------------------------------ derived bounds
@pytest.mark.parametrize("name", ["honest", "far_row", "garbage_row", "majority_bad"])
@pytest.mark.parametrize("P", [3, 8])
def test_bounds_the_rule_promises(name, P):
    bps = 64  # m = 8192
    m = bps * BLOCK
    rec, mask = family(name, P, bps)
    K = bin(mask).count("1")
    L = 3
    # absolute tau: every update is the mean of K vectors of norm at most tau, so L updates move the centre by at most
    # L tau from the start; the margin covers the fp32 roundoff of the sums (m 2^-24 <= 2^-11 at m = 8192)
    tau = clipping_tau(rec, mask, m)
    got, w, bad, info = reference(rec, mask, m, tau, L)
    start, res = info["centres"][0].double(), info["result"].double()
    fin = torch.isfinite(start)
    moved = float((res[fin] - start[fin]).norm())
    print(f"[q8 cclip bound] {name} P={P} tau={tau:.6g} moved={moved:.6g} bound={L * tau:.6g}")
    assert moved <= L * tau * (1 + 2.0 ** -8)
    assert torch.isfinite(decoded(got.unsqueeze(0))).all()
    # adaptive tau: the (K-1)//2-th smallest distance is the radius, so that many + 1 voters are inside it
    got, w, bad, info = reference(rec, mask, m, 0.0, L)
    assert sum(1 for x in w.tolist() if x == 1.0) >= (K - 1) // 2 + 1, w.tolist()
    assert torch.isfinite(decoded(got.unsqueeze(0))).all()
    if name == "garbage_row":
        assert float(w[P // 2]) == 0.0  # non-finite values where the centre is finite
    # one row with one NaN scale: weight 0, whatever else it sends
    one, _ = family("honest", P, bps)
    sc = scales_of(one)[1].view(torch.int32).tolist()
    sc[5] = NAN
    set_scales(one, 1, [x & 0xFFFFFFFF for x in sc])
    got, w, bad, _ = reference(one, mask, m, 0.0, L)
    assert float(w[1]) == 0.0 and int(bad) == 0 and torch.isfinite(decoded(got.unsqueeze(0))).all()


def _encode_rows(x: torch.Tensor) -> torch.Tensor:
    return torch.stack([pack(*q8_quantise(r.view(-1, BLOCK))) for r in x])


def test_what_the_rule_buys_over_q8():
    """Relative l2 distance from the honest mean, 8 peers, 2 attackers, five seeds: centered clipping over q8, the
    median over q8, centered clipping uncompressed (bf16 rows). The table is a measurement (README, Centered clipping);
    asserted is only what is derived: without an attacker the q8 record lies within half a code step, per element of
    its block, of the uncompressed rule on the same decoded rows. The margin 2^-12 of a step covers the codec's fp32
    roundoff: v * inv, inv and scale are each rounded once, 127 codes times 3 * 2^-24 is below 2^-15 of a step."""
    K, m = 8, 8192
    mask = (1 << K) - 1
    table = {}
    for kind in ATTACKS:
        acc = np.zeros(3)
        for seed in range(5):
            x, hmean, att = attacked(honest_rows(seed, K, m), kind)
            if kind == "nan":  # what a faulty peer can put on the wire: NaN scales
                rec = _encode_rows(torch.where(torch.isnan(x), torch.zeros_like(x), x))
                for k in att:
                    set_scales(rec, k, [NAN] * (m // BLOCK))
            else:
                rec = _encode_rows(x)
            got, w, bad, info = reference(rec, mask, m, 0.0, 3)
            cq = decoded(got.unsqueeze(0))[0]
            med = decoded(Quant8Compressor.reduce_robust_reference(rec.reshape(-1), K, (K - 1) // 2, mask, m)[0]
                          .unsqueeze(0))[0]
            unc = robust.centered_clip_reference(x.to(BF), mask, 0.0, 3)[0].float()
            unc = torch.where(torch.isfinite(unc), unc, torch.zeros_like(unc))
            acc += [rel_l2(cq, hmean), rel_l2(med, hmean), rel_l2(unc, hmean)]
            if kind == "none":
                ref = robust.centered_clip_reference(_canonical_decoded(rec), mask, 0.0, 3)[0]
                step = scales_of(got.unsqueeze(0))[0].repeat_interleave(BLOCK)
                assert int(bad) == 0 and w.tolist() == pytest.approx([1.0] * K, abs=0.5)
                assert bool(((cq - ref).abs().double() <= 0.5 * (1 + 2.0 ** -12) * step.double()).all())
        table[kind] = acc / 5
    print("\n[q8 cclip] rel. l2 from the honest mean: attack  cclip-q8  median-q8  cclip-bf16")
    for kind, a in table.items():
        print(f"[q8 cclip] {kind:7s} {a[0]:.4f} {a[1]:.4f} {a[2]:.4f}")


# ------------------------------------------------------------------------------ trainer and CLI
def _lone_trainer(**kw):
    from distributedvolunteercomputing_amd.models.mlp import MLP
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer

    cfg = LocalSGDConfig(H=1, comm_dtype=BF, **kw)
    return LocalSGDTrainer(MLP(seed=0), cfg, device="cpu")


def test_switches():
    from distributedvolunteercomputing_amd.jobs import train
    from distributedvolunteercomputing_amd.parallel.compression import PowerSGDCompressor, TopKCompressor
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig

    assert LocalSGDConfig().cclip_q8 is False
    tr = _lone_trainer(aggregate="cclip", cclip_q8=True)
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    tr.sync()  # accepted (alone: nothing to aggregate)
    for asked in (False, True):  # the old refusals with the switch off; robust_q8 is not the switch
        tr = _lone_trainer(aggregate="cclip", robust_q8=asked)
        tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
        with pytest.raises(ValueError, match="Quant8Compressor.*cclip_q8"):
            tr.sync()
    for make in (lambda t: TopKCompressor(t.flat.numel, 0.01, "cpu"), lambda t: PowerSGDCompressor(t.flat, 2, "cpu")):
        tr = _lone_trainer(aggregate="cclip", cclip_q8=True)  # the switch makes no other compressor legal
        tr.compressor = make(tr)
        with pytest.raises(ValueError, match="cannot be combined"):
            tr.sync()
    tr = _lone_trainer(aggregate="cclip", cclip_q8=True, algo="rccl")
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    with pytest.raises(ValueError, match="direct"):
        tr.sync()
    tr = _lone_trainer(aggregate="trimmed", cclip_q8=True)  # the switch is cclip's alone
    tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    with pytest.raises(ValueError, match="robust_q8"):
        tr.sync()
    a = train.parse(["--aggregate", "cclip", "--compression", "q8", "--clip-q8", "--byzantine", "nan"])
    assert (a.aggregate, a.compression, a.clip_q8) == ("cclip", "q8", True)
    assert train.parse([]).clip_q8 is False
    for argv in (["--aggregate", "cclip", "--compression", "q8"],
                 ["--clip-q8"],
                 ["--aggregate", "cclip", "--clip-q8"],
                 ["--aggregate", "median", "--compression", "q8", "--clip-q8"],
                 ["--aggregate", "cclip", "--compression", "topk", "--clip-q8"],
                 ["--aggregate", "cclip", "--compression", "powersgd"],
                 ["--aggregate", "cclip", "--compression", "q8", "--clip-q8", "--algo", "ring"],
                 ["--trainer", "sharded", "--aggregate", "cclip", "--compression", "q8", "--clip-q8"]):
        with pytest.raises(SystemExit):
            train.parse(argv)


def test_the_cli_names_the_flag(capsys):
    from distributedvolunteercomputing_amd.jobs import train

    with pytest.raises(SystemExit):
        train.parse(["--aggregate", "cclip", "--compression", "q8"])
    assert "--clip-q8" in capsys.readouterr().err


# ------------------------------------------------------------------------------ a real round
_TAU, _ITERS = 0.0, 3


def _round_worker(rank, world, port):
    from distributedvolunteercomputing_amd.jobs.train import nan_scales
    from distributedvolunteercomputing_amd.models.mlp import MLP, synthetic_mnist
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer
    from distributedvolunteercomputing_amd.parallel.peer_group import PeerGroup

    g = PeerGroup(_mp.make_store(rank, world, port), rank, world, "gloo")
    cfg = LocalSGDConfig(H=1000, lr=0.05, weight_decay=0.0, max_grad_norm=0.0, comm_dtype=BF, aggregate="cclip",
                         clip_tau=_TAU, clip_iters=_ITERS, cclip_q8=True)
    tr = LocalSGDTrainer(MLP(seed=0), cfg, group=g, device="cpu")
    comp = tr.compressor = Quant8Compressor(tr.flat.numel, "cpu")
    if rank == 1:
        tr.wire_hook = nan_scales
    x, y = synthetic_mnist(512, seed=rank)
    P = world
    out = {"rounds": [], "losses": [], "n": tr.flat.numel}
    for rnd, newcomers in enumerate(((), (2,), ())):  # rank 2 comes back untrained in the second round and does not vote
        for i in range(2):
            b = slice(((2 * rnd + i) % 8) * 64, ((2 * rnd + i) % 8 + 1) * 64)
            out["losses"].append(float(tr.step(x[b], y[b]).extra["loss_t"]))
        if rank in newcomers:
            tr.master.copy_(tr.anchor)  # what an admitted newcomer holds: the group's model, an all-zero delta
        tr._apply(tr._reduce(newcomers))
        out["rounds"].append({"wire": comp._buf(P, "wire").numpy().tobytes(),
                              "gathered": comp._buf(P, "gathered").numpy().tobytes(),
                              "w": list(tr.clip_weight), "share": tr.nonfinite_share})
    g.barrier()
    out["anchor"] = hashlib.sha256(tr.anchor.numpy().tobytes()).hexdigest()
    out["param"] = hashlib.sha256(tr.flat.param.view(torch.int16).numpy().tobytes()).hexdigest()
    out["finite"] = bool(torch.isfinite(tr.anchor).all())
    out["sent"] = comp.bytes_sent
    return out


def test_a_real_gloo_round_is_the_reference_on_the_wire_records():
    P = 4
    res = _mp.run(_round_worker, P)
    assert len({r["anchor"] for r in res.values()}) == 1 and len({r["param"] for r in res.values()}) == 1
    n = res[0]["n"]
    L, m, rec = Quant8Compressor(n, "cpu").layout(P)
    for rnd, live in enumerate((None, [0, 1, 3], None)):
        mask = robust.mask_of(live, P)
        wires = [torch.frombuffer(bytearray(res[r]["rounds"][rnd]["wire"]), dtype=torch.uint8).view(P, rec)
                 for r in range(P)]
        records, wsum, bad = [], torch.zeros(P, dtype=torch.float64), 0
        for j in range(P):
            recv = torch.stack([wires[r][j] for r in range(P)])
            out, w, b, _ = reference(recv, mask, min(max(n - j * m, 0), m), _TAU, _ITERS)
            records.append(out)
            wsum += w.double()
            bad += int(b)
        want_w = (wsum / P).float().tolist()
        for r in range(P):
            got = res[r]["rounds"][rnd]
            assert got["gathered"] == torch.cat(records).numpy().tobytes(), (rnd, r)
            assert got["w"] == want_w and got["share"] == bad / n, (rnd, r, got["w"], want_w)
            assert got["w"][1] == 0.0  # the peer with NaN scales
        if live is not None:
            assert want_w[2] == 0.0  # the newcomer does not vote
    for r in range(P):
        assert res[r]["finite"] and res[r]["sent"] == 3 * (2 * (P - 1) * rec + 8 * (P + 1))
        if r != 1:
            assert all(math.isfinite(l) for l in res[r]["losses"]), res[r]["losses"]


def test_alone_is_one_record_of_the_own_values():
    n = 128 * 7 + 45
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g))).to(BF)
    comp, ref = Quant8Compressor(n, "cpu"), Quant8Compressor(n, "cpu")
    avg, w, bad = comp.allreduce_cclip(x, None, 0.0, 3)
    assert torch.equal(avg.view(torch.int16), ref.allreduce_mean(x, None).view(torch.int16))
    assert w.tolist() == [1.0] and bad == 0 and torch.equal(comp.e, ref.e)


# ------------------------------------------------------------------------------ an aborted round
def _sim_round(comps, xs, mask):
    """One round in one process: encode on every peer, shuffle the records by hand, reduce_cclip on every owner."""
    P = len(comps)
    n = comps[0].n
    L, m, rec = comps[0].layout(P)
    wires = [comps[r].encode(xs[r], P).view(P, rec).clone() for r in range(P)]
    records = []
    for j in range(P):
        recv = torch.stack([wires[r][j] for r in range(P)]).reshape(-1)
        records.append(comps[j].reduce_cclip(recv, P, mask, min(max(n - j * m, 0), m), 0.0, 3).clone())
    return torch.cat(records)


def test_an_aborted_round_restored_and_redone_is_a_clean_round():
    P, n = 3, 128 * 7 + 45
    g = torch.Generator().manual_seed(11)
    xs = [[(torch.randn(n, generator=g) * 0.1).to(BF) for _ in range(P)] for _ in range(2)]
    clean = [Quant8Compressor(n, "cpu") for _ in range(P)]
    want = [_sim_round(clean, xs[0], 0b111), _sim_round(clean, xs[1], 0b111)]
    comps = [Quant8Compressor(n, "cpu") for _ in range(P)]
    assert torch.equal(_sim_round(comps, xs[0], 0b111), want[0])
    snaps = [c.snapshot() for c in comps]
    for r in range(P):
        comps[r].encode(xs[1][r], P)  # the aborted round got as far as the encode: e has moved
    assert any(not torch.equal(c.e, s["e"]) for c, s in zip(comps, snaps))
    for c, s in zip(comps, snaps):
        c.restore(s)
    assert torch.equal(_sim_round(comps, xs[1], 0b111), want[1])
    for c, d in zip(comps, clean):
        assert torch.equal(c.e, d.e)


# ------------------------------------------------------------------------------ the CLI end to end
def _cli_worker(rank, world, port, metrics):
    from distributedvolunteercomputing_amd.jobs import train

    argv = ["--model", "mlp", "--steps", "12", "--H", "2", "--batch", "32", "--lr", "0.05", "--backend", "gloo",
            "--peer-id", str(rank), "--world", str(world), "--store-port", str(port), "--log-every", "2",
            "--aggregate", "cclip", "--compression", "q8", "--clip-q8", "--metrics", f"{metrics}.{rank}"]
    if rank == world - 1:
        argv += ["--byzantine", "nan"]  # under q8: NaN into every scale of its wire records
    return train.main(argv)


def test_train_cli_cclip_q8_with_a_nan_peer(tmp_path):
    base = str(tmp_path / "m.jsonl")
    res = _mp.run(_cli_worker, 4, base)
    assert all(v == 0 for v in res.values())
    recs = [json.loads(l) for l in open(base + ".0")]
    assert len(recs) == 6 and all(math.isfinite(r["loss"]) for r in recs)
    assert recs[-1]["loss"] < recs[0]["loss"]
    assert all(len(r["clip_weight"]) == 4 and r["clip_weight"][3] == 0.0 for r in recs)
    assert all(w > 0 for r in recs for w in r["clip_weight"][:3])
    assert all(r["nonfinite_share"] == 0 for r in recs)
