"""Sharded data-parallel training: ZeRO-1 optimizer-state sharding across volunteer peers,
R-fold replication of every shard, optional gradient compression, elastic re-shard, and
mid-collective failure recovery.

Per step (all on the GPU stream):
  fwd/bwd -> flat bf16 grads -> averaged gradient of the shards this peer holds
  (uncompressed: ONE reduce-scatter + R ring-shifts of the averaged shard to its replica
  holders — 1.125x the gradient bytes at P=8, R=2, instead of an all-reduce's 1.75x;
  compressed: PowerSGD / top-k with error feedback) -> grad-norm kernel -> fused AdamW on MY
  shard and on the R shards I replicate -> all-gather of the updated bf16 param shards.

Fault tolerance: shard j is held by peer j (primary) and peers j+1 .. j+R (replicas, default
R = 2, so BASELINE.json config 4's "kill 2 mid-training" — any two peers, adjacent or not —
never loses fp32 optimizer state). Replicas apply the very same AdamW update from the same
averaged gradient: no extra traffic per step beyond the ring-shifts; only (1+R)x the
HBM-bound optimizer work on (1+R)/P of the model. When the membership changes the survivors
re-shard point to point: each slice of the new layout a peer must hold comes from one live old
holder (or its own old shards), in one variable-split all-to-all; only the slices that change
holder travel and nothing is materialised at full-model size. If a shard has no live holder left the re-shard fails loudly (StateLost)
unless ``allow_state_loss`` is set. Under elastic membership every collective phase runs
guarded (parallel/elastic.py): a peer dying inside the gradient reduction or the parameter
gather aborts the phase on all survivors, which recover to a new generation, re-shard, and
redo the reduction (the local gradients are intact: collectives never write into them) or
rebuild the parameters from the re-sharded fp32 masters.

No reference analog: SURVEY.md §2.7 "Optimizer-state sharding (ZeRO-like)" and §2.9
"Optimizer-state sharding + elastic re-shard" (BASELINE.json configs 4 and 5).
"""
from __future__ import annotations

import time
from dataclasses import dataclass

import torch

from .. import ops
from ..ops.optim import OS_SUMSQ
from .collectives import allreduce_sum_
from .flat_params import FlatBuffers, FlatParams
from .local_sgd import mean_slice, restore_extras
from .peer_group import PeerFailure


class StateLost(RuntimeError):
    """Every holder of some optimizer-state shard left the job at once."""


@dataclass
class ShardedConfig:
    lr: float = 3e-4
    betas: tuple = (0.9, 0.95)
    eps: float = 1e-8
    weight_decay: float = 0.1
    max_grad_norm: float = 1.0
    replicas: int = 2  # extra holders of every shard (peers r+1 .. r+replicas)
    replicate: bool = True  # False: no replicas (replicas = 0)
    algo: str = "rs"  # rs (reduce-scatter + replica shifts) | rccl | rs_ag | butterfly | ring | direct
    allow_state_loss: bool = False  # restart a lost shard from the bf16 params instead of raising
    # fp32: m and v in fp32 (12 B/param with the master) | compact: fp8 m and fp16 v with one exponent
    # per 32 elements (7.06 B/param; ops/optim.py CompactState). Re-shard pieces and checkpoints are fp32
    # either way; every held shard (primary or replica) keeps "cs" in place of "m" and "v"
    opt_state: str = "fp32"


class ShardedDPTrainer:
    def __init__(self, model, cfg: ShardedConfig, *, group=None, membership=None, compressor=None, device=None):
        self.model = model
        self.cfg = cfg
        self.device = torch.device(device or next(model.parameters()).device)
        if cfg.opt_state not in ("fp32", "compact"):
            raise ValueError(f"opt_state must be 'fp32' or 'compact', got {cfg.opt_state!r}")
        self.compact = cfg.opt_state == "compact"
        if self.compact:
            ops.check_compact_betas(cfg.betas)
        self.flat = FlatParams(model, device=self.device)
        self.buffers = FlatBuffers(model)
        self.membership = membership
        self.group = membership.group if membership is not None else group
        self.compressor = compressor
        self.ostate = ops.new_ostate(self.device, cfg.lr)
        self.t = 0
        self.reshard_events = []
        self.failed_phases = 0
        self._skip_round = False
        self._sumsq = None  # global squared gradient norm from the reduce-scatter path
        self._layout_members = list(self.group.members) if self.group is not None else [0]
        self._layout(full_master=self.flat.param, full_m=None, full_v=None)  # slices converted one by one

    # ------------------------------------------------------------------ layout
    @property
    def world(self):
        return 1 if self.group is None else self.group.size

    @property
    def rank(self):
        return 0 if self.group is None else self.group.rank

    @property
    def n_replicas(self):
        if not self.cfg.replicate:
            return 0
        return max(0, min(self.cfg.replicas, self.world - 1))

    def _layout(self, full_master, full_m, full_v):
        P, r = self.world, self.rank
        lo, hi = self.flat.shard_bounds(r, P)
        self.prim = (lo, hi)

        def cut(full, a, b):
            if full is None:
                return torch.zeros(b - a, dtype=torch.float32, device=self.device)
            return full[a:b].to(torch.float32, copy=True)

        def moments(a, b):
            if not self.compact:
                return {"m": cut(full_m, a, b), "v": cut(full_v, a, b)}
            if full_m is None and full_v is None:
                return {"cs": ops.CompactState.zeros(b - a, self.device)}
            return {"cs": ops.CompactState.from_fp32(cut(full_m, a, b), cut(full_v, a, b))}

        self.master = cut(full_master, lo, hi)
        self._set_moments(moments(lo, hi))
        self.reps = []  # replicas: shards (r-1) .. (r-R) of the current layout
        for i in range(1, self.n_replicas + 1):
            j = (r - i) % P
            a, b = self.flat.shard_bounds(j, P)
            self.reps.append({"shard": j, "range": (a, b), "master": cut(full_master, a, b), **moments(a, b)})

    def _set_moments(self, d):
        """The primary's moments: fp32 `m`, `v`, or the compact `cs` (then m and v are None)."""
        self.m, self.v, self.cs = d.get("m"), d.get("v"), d.get("cs")

    def _held(self):
        """Every shard this peer holds, the primary first, as dicts like the entries of `reps`."""
        mom = {"cs": self.cs} if self.compact else {"m": self.m, "v": self.v}
        return [{"shard": self.rank, "range": self.prim, "master": self.master, **mom}] + self.reps

    @property
    def back(self):  # first replica's range (compat)
        return self.reps[0]["range"] if self.reps else None

    def checkpoint_slice(self):
        lo, hi = self.prim
        m, v = self.cs.to_fp32() if self.compact else (self.m, self.v)  # the file holds fp32 either way
        t = {"master": self.master, "m": m, "v": v}
        if self.compressor is not None:
            t["ef"] = mean_slice(self.group, self.compressor.state_dict()["ef"], lo, hi)
        return lo, hi, t

    def checkpoint_global(self) -> dict:
        out = {}
        if self.buffers:
            out["buffers"] = self.buffers.as_fp32()
        if self.compressor is not None and "Q" in self.compressor.state_dict():
            out["psgd_Q"] = self.compressor.state_dict()["Q"]
        return out

    def restore(self, reader):
        """Load a checkpoint written by any number of peers into the CURRENT layout."""
        reader.check_layout(self.flat)
        dev = self.device
        param, ost = reader.params()
        self.flat.param.copy_(param.to(dev))
        self.ostate.copy_(ost.to(dev))
        for h in self._held():
            a, b = h["range"]
            h["master"].copy_(reader.read_range("master", a, b).to(dev))
            m, v = reader.read_range("m", a, b).to(dev), reader.read_range("v", a, b).to(dev)
            if self.compact:
                h["cs"].load_fp32(m, v)
            else:
                h["m"].copy_(m)
                h["v"].copy_(v)
        restore_extras(self, reader)
        self.t = reader.step

    def state_bytes(self) -> int:
        """Bytes of optimizer state (master and moments) of every shard this peer holds."""
        n = 0
        for h in self._held():
            n += 4 * h["master"].numel() + (h["cs"].nbytes if self.compact else 8 * h["master"].numel())
        return n

    # ------------------------------------------------------------------ step
    def step(self, x, y):
        mem = self.membership
        if mem is not None and not self._skip_round:
            grp, changed, newcomers = mem.sync_round()
            if changed:
                self._reshard_until_ok(grp, newcomers)
        self._skip_round = False
        self.flat.zero_grad()
        loss = self.model(x, y)
        loss.backward()
        g = self.flat.grad
        if mem is None:
            avg = self._average(g)
            self._adam(avg)
            self._gather_params(elastic=False)
            self.buffers.average_(self.group)
        else:
            while True:
                snap = self.compressor.snapshot() if (self.compressor is not None and self.world > 1) else None
                try:
                    with mem.guard("g"):
                        avg = self._average(g)
                    break
                except PeerFailure:
                    if snap is not None:
                        self.compressor.restore(snap)
                    self.failed_phases += 1
                    grp, _, newcomers = mem.recover()
                    self._reshard_until_ok(grp, newcomers)
            self._adam(avg)
            try:
                with mem.guard("p"):
                    params = self._gather_params(elastic=True)
                    bufs = self.buffers.averaged(self.group)
                if params is not None:  # applied only after the phase committed
                    self.flat.param.copy_(params)
                if bufs is not None:
                    self.buffers.load_fp32(bufs)
            except PeerFailure:
                self.failed_phases += 1
                grp, _, newcomers = mem.recover()
                self._reshard_until_ok(grp, newcomers)  # also re-gathers exact bf16 parameters
                # the re-shard ran this step's membership round: the next step must not run
                # another one (a peer admitted in the recovery goes straight into the gradient
                # phase, as join_running_job() arranges), or the two sides wait on different
                # rounds until a process-group timeout
                self._skip_round = True
        self.t += 1
        return loss.detach()

    def _average(self, g):
        """Averaged gradient for (at least) every shard this peer holds, in a fresh flat buffer
        (collectives never write into the live gradient, so an aborted phase can be redone)."""
        P = self.world
        self._sumsq = None
        if self.compressor is not None:
            return self.compressor.allreduce_mean(g, self.group)
        if P == 1:
            return g
        n = g.numel()
        algo = self.cfg.algo
        if algo == "rs" and n % P == 0 and self.prim[1] - self.prim[0] == n // P:
            avg = torch.empty_like(g)
            lo, hi = self.prim
            self.group.reduce_scatter_(avg[lo:hi], g)
            mine = avg[lo:hi]
            mine.div_(P)
            for i in range(1, self.n_replicas + 1):  # ring-shift the averaged shard to its replicas
                j = (self.rank - i) % P
                a, b = self.flat.shard_bounds(j, P)
                self.group.exchange_all(mine, avg[a:b], (self.rank + i) % P, j)
            if self.cfg.max_grad_norm > 0:  # global norm from the per-shard squared sums
                sq = torch.linalg.vector_norm(mine, dtype=torch.float32).square().reshape(1)
                self.group.allreduce_(sq)
                self._sumsq = sq
            return avg
        avg = g.clone()
        allreduce_sum_(avg, self.group, "rccl" if algo == "rs" else algo)
        return avg.div_(P)

    def _adam_range(self, avg, a, b, master, m, v, cs=None):
        c = self.cfg
        n_decay = max(0, min(self.flat.n_decay - a, b - a))
        n_decay -= n_decay % 8
        # the flat kernels read ostate (step/lr/clip) — shared by all ranges, prologue once
        C = ops.native() if self.flat.param.is_cuda else None
        if cs is not None:
            # primary and replicas run the same kernel on the same bytes, so they stay bit-identical
            ops.adamw_flat_compact(self.flat.param[a:b], avg[a:b], master, cs, self.ostate, n_decay=n_decay,
                                   beta1=c.betas[0], beta2=c.betas[1], eps=c.eps, wd=c.weight_decay)
        elif C is not None:
            C.adamw_flat(self.flat.param[a:b], avg[a:b], master, m, v, n_decay, self.ostate, c.betas[0], c.betas[1],
                         c.eps, c.weight_decay)
        else:
            from ..ops.optim import adamw_step

            st = self.ostate.clone()
            st[0] -= 1  # the reference increments step itself
            adamw_step(self.flat.param[a:b], avg[a:b], master, m, v, st, n_decay=n_decay, beta1=c.betas[0],
                       beta2=c.betas[1], eps=c.eps, wd=c.weight_decay, max_norm=0.0)

    def _held_ranges(self):
        return [self.prim] + [rep["range"] for rep in self.reps]

    def _adam(self, avg):
        """Local AdamW on every held shard (no communication: the global gradient norm of the
        reduce-scatter path was all-reduced inside the guarded gradient phase)."""
        c = self.cfg
        sumsq, self._sumsq = self._sumsq, None
        if avg.is_cuda:
            C = ops.native()
            if c.max_grad_norm > 0:
                if sumsq is not None:
                    self.ostate[OS_SUMSQ : OS_SUMSQ + 1].copy_(sumsq)
                else:
                    self.ostate[OS_SUMSQ].zero_()
                    C.grad_sumsq(avg, self.ostate)
            C.adam_prologue(self.ostate, float(c.max_grad_norm))
        else:
            self.ostate[0] += 1
            coef = 1.0
            if c.max_grad_norm > 0:
                nrm = float(sumsq.sqrt()) if sumsq is not None else avg.float().norm().item()
                coef = min(1.0, c.max_grad_norm / (nrm + 1e-6))
            self.ostate[2] = coef
            if coef != 1.0:
                avg = (avg.float() * coef).to(avg.dtype)
                self.ostate[2] = 1.0
        for h in self._held():
            a, b = h["range"]
            self._adam_range(avg, a, b, h["master"], h.get("m"), h.get("v"), h.get("cs"))

    def _gather_params(self, elastic: bool):
        """All-gather of the updated bf16 primaries. Elastic: into a fresh buffer that the caller
        copies into the parameters only after the phase's verdict is `commit`."""
        if self.world == 1:
            return None
        lo, hi = self.prim
        mine = self.flat.param[lo:hi].clone()
        if not elastic:
            self.group.all_gather_(self.flat.param, mine)
            return None
        out = torch.empty_like(self.flat.param)  # never let an aborted gather write the params
        self.group.all_gather_(out, mine)
        return out

    def _refresh_params(self):
        """bf16 parameters of every slice this peer holds, from its fp32 masters."""
        for (a, b), master in [(self.prim, self.master)] + [(r["range"], r["master"]) for r in self.reps]:
            if b > a:
                if master.is_cuda:
                    ops.f32_to_bf16(master, self.flat.param[a:b])
                else:
                    self.flat.param[a:b].copy_(master)

    # ------------------------------------------------------------------ elastic re-shard
    def join_running_job(self):
        """A newly admitted peer takes part in the re-shard that admitted it (it holds no
        shard, so it only receives); its first step then skips the membership round, which
        the continuing members already ran."""
        self._layout_members = []
        mem = self.membership
        self._reshard_until_ok(mem.group, mem.newcomers)
        self._skip_round = True

    def _reshard_until_ok(self, grp, newcomers):
        mem = self.membership
        while True:
            try:
                with mem.guard("s"):
                    new_state = self._reshard_collect(grp, newcomers)
                self._reshard_apply(grp, *new_state)
                return
            except PeerFailure:
                self.failed_phases += 1
                grp, _, newcomers = mem.recover()

    def reshard(self, new_group, newcomers=()):
        """Non-elastic entry point (tests / manual regroup)."""
        self._reshard_apply(new_group, *self._reshard_collect(new_group, newcomers))

    def _reshard_plan(self, L, R_old, members, R_new, newcomers):
        """Where every piece of the NEW layout comes from. For each member d of the new group and
        each shard it must hold (its primary and R_new replicas), the intersections with the OLD
        layout's shards: (d, k (index among d's held shards), src pid, old shard j, [x, y)).
        src is d itself when d held old shard j (a local copy), else one live old holder of j,
        chosen round-robin over the holders so the senders share the load. Pieces whose old
        shard has no live holder are returned as lost. Identical on every member."""
        old_P, new_P = len(L), len(members)
        live = {}
        for j in range(old_P):
            hs = [L[(j + i) % old_P] for i in range(R_old + 1)]
            live[j] = [h for h in hs if h in members and h not in newcomers]
        old_bounds = [self.flat.shard_bounds(j, old_P) for j in range(old_P)]
        plan, lost = [], []
        for d, pid in enumerate(members):
            held = [d] + [(d - i) % new_P for i in range(1, R_new + 1)]
            for k, sh in enumerate(held):
                a, b = self.flat.shard_bounds(sh, new_P)
                for j, (aj, bj) in enumerate(old_bounds):
                    x, y = max(a, aj), min(b, bj)
                    if y <= x:
                        continue
                    H = live[j]
                    if not H:
                        lost.append((d, k, x, y))
                        continue
                    src = pid if pid in H else H[(d + j) % len(H)]
                    plan.append((d, k, src, j, x, y))
        return plan, lost

    def _reshard_collect(self, new_group, newcomers):
        """Targeted re-shard: every slice of optimizer state (fp32 master, m, v)
        that a member must hold in the NEW layout is assembled from pieces of the OLD layout; a
        piece it already holds is copied locally, every other piece comes from ONE live old
        holder, point to point, all of it in ONE variable-split all-to-all (RCCL: grouped
        send/recv over the xGMI links). Nothing is materialised at full-model size (the previous
        scheme rebuilt the full 12 B/param state on every peer: 96 GB per peer and per regroup at
        8B parameters); the wire carries exactly the state of the slices that change holder.
        Newcomers additionally get the bf16 parameters from an all-gather of the new primaries'
        masters. Touches no trainer state: the result is applied only after the phase commits."""
        t0 = time.perf_counter()
        members = list(new_group.members)
        my_pid = self.membership.pid if self.membership is not None else members[new_group.rank]
        cont = [i for i, m in enumerate(members) if m not in newcomers]
        if not cont:
            raise StateLost("no member of the new generation holds optimizer state")
        root0 = cont[0]
        dev = self.device
        cdev = dev if new_group.backend == "nccl" else torch.device("cpu")
        # the layout that the continuing members' shards follow (newcomers do not know it)
        hdr = torch.full((257,), -1, dtype=torch.int64, device=cdev)
        if new_group.rank == root0:
            L = self._layout_members
            hdr[0] = len(L)
            hdr[1 : 1 + len(L)] = torch.tensor(L, dtype=torch.int64)
        new_group.broadcast_(hdr, root=root0)
        hdr = hdr.cpu()
        L = [int(x) for x in hdr[1 : 1 + int(hdr[0])]]
        old_P, new_P = len(L), len(members)
        R_old = min(self.cfg.replicas if self.cfg.replicate else 0, old_P - 1)
        R_new = max(0, min(self.cfg.replicas, new_P - 1)) if self.cfg.replicate else 0
        plan, lost = self._reshard_plan(L, R_old, members, R_new, newcomers)
        if lost and not self.cfg.allow_state_loss:
            raise StateLost(f"optimizer-state ranges {[(x, y) for *_, x, y in lost]} had no live holder among "
                            f"{members} (old layout {L}, replicas {R_old})")
        me = new_group.rank
        my_old = L.index(my_pid) if (my_pid in L and my_pid not in newcomers) else None
        held = [me] + [(me - i) % new_P for i in range(1, R_new + 1)]
        dst = []  # this peer's new (primary, replicas): fresh tensors, live state untouched
        for sh in held:
            a, b = self.flat.shard_bounds(sh, new_P)
            dst.append({"shard": sh, "range": (a, b),
                        **{f: torch.zeros(b - a, dtype=torch.float32, device=dev) for f in ("master", "m", "v")}})

        def old_piece(j, x, y):
            # fp32 (master, m, v) of [x, y). Compact: decoded piece by piece (nothing at full-shard size);
            # pieces start and end on multiples of ALIGN = 64 elements, so whole 32-element blocks
            # travel and the destination's encode gives back the very same bytes
            st = self._shard_state_old(j, my_old, old_P)
            aj = self.flat.shard_bounds(j, old_P)[0]
            if self.compact:
                return [st["master"][x - aj : y - aj], *st["cs"].to_fp32(x - aj, y - aj)]
            return [st[f][x - aj : y - aj] for f in ("master", "m", "v")]

        send = [[] for _ in range(new_P)]
        recv = [[] for _ in range(new_P)]
        for d, k, src, j, x, y in plan:
            if members[d] == my_pid and src == my_pid:
                a = dst[k]["range"][0]
                for f, t in zip(("master", "m", "v"), old_piece(j, x, y)):
                    dst[k][f][x - a : y - a].copy_(t)
            elif src == my_pid:
                send[d].extend(old_piece(j, x, y))
            elif members[d] == my_pid:
                recv[members.index(src)].append((k, x, y))
        send_splits = [sum(t.numel() for t in parts) for parts in send]
        recv_splits = [3 * sum(y - x for _, x, y in pieces) for pieces in recv]
        moved = 0
        if sum(send_splits) or sum(recv_splits) or new_P > 1:
            sbuf = (torch.cat([t.to(cdev) for parts in send for t in parts]) if sum(send_splits)
                    else torch.zeros(0, dtype=torch.float32, device=cdev))
            rbuf = torch.empty(sum(recv_splits), dtype=torch.float32, device=cdev)
            if new_P > 1:
                new_group.alltoall_(rbuf, sbuf, recv_splits, send_splits)
            pos = 0
            for src_rank in range(new_P):
                for k, x, y in recv[src_rank]:
                    a = dst[k]["range"][0]
                    for f in ("master", "m", "v"):
                        dst[k][f][x - a : y - a].copy_(rbuf[pos : pos + y - x].to(dev))
                        pos += y - x
            moved = 4 * sum(send_splits)
        changed = 12 * sum(y - x for pieces in recv for _, x, y in pieces)
        ost = self.ostate.clone()
        new_group.broadcast_(ost, root=root0)  # step counter / lr must agree
        bufs = None
        if self.buffers:
            bufs = self.buffers.as_fp32().to(cdev)
            new_group.broadcast_(bufs, root=root0)
        params = None
        if new_P > 1:
            # exact bf16 parameters for everyone from the new primaries' masters (newcomers hold
            # none; after an aborted parameter gather the survivors' copies are one step stale)
            for d, k, x, y in lost:
                if members[d] == my_pid:  # allow_state_loss: restart from the bf16 params we have
                    a = dst[k]["range"][0]
                    dst[k]["master"][x - a : y - a].copy_(self.flat.param[x:y].float())
            lo, hi = dst[0]["range"]
            mine = torch.empty(hi - lo, dtype=self.flat.param.dtype, device=dev)
            ops.f32_to_bf16(dst[0]["master"], mine) if mine.is_cuda else mine.copy_(dst[0]["master"])
            params = torch.empty_like(self.flat.param)
            new_group.all_gather_(params, mine)
        if self.compact:  # the assembled fp32 moments of every destination shard go back to the compact format
            for h in dst:
                h["cs"] = ops.CompactState.from_fp32(h.pop("m"), h.pop("v"))
        ev = {"t": self.t, "old": L, "new": members, "lost": [(x, y) for *_, x, y in lost],
              "bytes_sent": moved, "bytes_changed": changed, "ms": (time.perf_counter() - t0) * 1e3}
        return dst, ost, bufs, params, lost, ev

    def _shard_state_old(self, j, my_old, old_P):
        """What this peer held for shard j of the OLD layout (index my_old of old_P): a dict as in `_held`."""
        if my_old is None:
            raise StateLost(f"asked for shard {j} but this peer held no shard")
        if j == my_old:
            return self._held()[0]
        for rep in self.reps:
            if rep["shard"] == j:
                return rep
        raise StateLost(f"shard {j} expected on this peer (old index {my_old} of {old_P})")

    def _reshard_apply(self, new_group, dst, ost, bufs, params, lost, ev):
        members = list(new_group.members)
        my_pid = self.membership.pid if self.membership is not None else members[new_group.rank]
        for d, k, x, y in lost:  # allow_state_loss: no live holder, restart from the bf16 params
            if members[d] == my_pid and params is None:
                a = dst[k]["range"][0]
                dst[k]["master"][x - a : y - a].copy_(self.flat.param[x:y].float())
        self.ostate.copy_(ost)
        if bufs is not None:
            self.buffers.load_fp32(bufs)
        self.group = new_group
        self._layout_members = members
        self.prim = dst[0]["range"]
        self.master = dst[0]["master"]
        self._set_moments(dst[0])
        self.reps = [dict(r) for r in dst[1:]]
        if params is not None:
            self.flat.param.copy_(params)
        else:  # a single survivor holds everything: its parameters from its masters
            self._refresh_params()
        self.reshard_events.append(ev)
