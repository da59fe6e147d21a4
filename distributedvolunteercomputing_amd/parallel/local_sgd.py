"""Local-SGD training engine for volunteer peers (one process per GPU).

Each peer runs H local AdamW steps on its own data shard, then the peers average their model
(BASELINE.json configs 1, 2, 4: "local-SGD H=4 + butterfly all-reduce", "kill 2 then rejoin").

Per-step GPU work (all on the current HIP stream, graph-capturable):
  zero flat grad -> fwd/bwd -> [grad-norm kernel] -> AdamW prologue -> fused flat AdamW.
Every H steps (`sync`):
  membership round (elastic only) -> lsgd_delta kernel (bf16 pseudo-gradient)
  -> [compression: top-k+EF, PowerSGD or q8+EF] -> all-reduce SUM over live peers
  -> lsgd_apply kernel (average + optional outer Nesterov momentum, writes anchor/master/param).
With ``aggregate="trimmed" | "median"`` the all-reduce SUM is replaced by a coordinate-wise trimmed
mean over the same exchange (collectives.robust_mean_), which survives peers that send wrong numbers.
The robust rules combine with q8 compression (on request: LocalSGDConfig.robust_q8) and with no other: the
q8 shard owner holds every peer's record of its shard before anything is summed, so its reduce kernel takes
the trimmed mean of the decoded records instead (Quant8Compressor.allreduce_robust).
``aggregate="cclip"`` is the per-peer rule over the same exchange (collectives.cclip_mean_): every shard owner
clips the peers' copies of its shard around their median, so one peer moves a shard's aggregate by at most
clip_iters * tau / K in l2 whatever it sends. It runs over `direct`, in this trainer only: uncompressed, or (on
request: LocalSGDConfig.cclip_q8) over the q8 exchange, where the shard owner clips the peers' decoded records and
quantises the aggregate again (Quant8Compressor.allreduce_cclip).

Reference analog: the chunk (100 frames) is the reference's unit of independent work
(worker.py:16, server.py:77-91); here the unit is H optimizer steps.
"""
from __future__ import annotations

import contextlib
import time
from dataclasses import dataclass, field

import torch

from .. import ops
from ..utils.trace import NULL_TRACER
from ..ops.robust import AGGREGATES, check_clip, effective_trim
from .collectives import allreduce_sum_, cclip_mean_, robust_mean_
from .compression import Quant8Compressor
from .flat_params import FlatBuffers, FlatParams
from .peer_group import PeerFailure


@dataclass
class LocalSGDConfig:
    lr: float = 6e-4
    betas: tuple = (0.9, 0.95)
    eps: float = 1e-8
    weight_decay: float = 0.1
    max_grad_norm: float = 1.0
    H: int = 4  # local steps between averaging rounds
    algo: str = "direct"  # direct | rccl | rs_ag | butterfly | ring (parallel/collectives.py)
    outer_lr: float = 1.0
    outer_momentum: float = 0.0
    nesterov: bool = False
    comm_dtype: torch.dtype = torch.bfloat16
    compression: str = "none"  # none | topk | powersgd | q8
    topk_ratio: float = 0.01
    powersgd_rank: int = 4
    # fp32: m and v in fp32 (12 B/param with the master) | compact: fp8 m and fp16 v with one exponent
    # per 32 elements (7.06 B/param; ops/optim.py CompactState); checkpoints hold fp32 either way
    opt_state: str = "fp32"
    # how the peers' pseudo-gradients become one: mean | trimmed | median. The robust rules
    # (ops/robust.py) drop the `trim` lowest and highest values of every coordinate (median: all but
    # the middle one or two), so up to `trim` peers per coordinate may send anything, NaN included
    # cclip: centered clipping, the per-peer rule (clip_tau: the clipping radius in the l2 norm of a shard, 0 =
    # each update's median distance; clip_iters: updates per round, 1..8)
    aggregate: str = "mean"
    trim: int = 1
    clip_tau: float = 0.0
    clip_iters: int = 3
    # let a robust rule run over the q8 exchange (Quant8Compressor.allreduce_robust). Off by default, so a robust
    # rule with any compressor is refused as before: over q8 the rule does not mean quite what it means on the
    # uncompressed pseudo-gradient (the aggregate is quantised again, and a coordinate whose aggregate is
    # non-finite comes out as 0 and is counted in nonfinite_share where the uncompressed rule hands on the NaN),
    # so the caller says that this is what it wants. `train --compression q8 --aggregate ...` says so
    robust_q8: bool = False
    # let centered clipping run over the q8 exchange (Quant8Compressor.allreduce_cclip). Off by default, so cclip with
    # any compressor is refused as before: over q8 the rule measures the peers' distances on their decoded 8-bit
    # records, the aggregate is quantised again, and a coordinate whose aggregate is non-finite (a non-finite centre:
    # more than half the voters sent one there) comes out as 0 and is counted in nonfinite_share where the
    # uncompressed rule hands on the NaN, so the caller says that this is what it wants. `train --aggregate cclip
    # --compression q8 --clip-q8` says so
    cclip_q8: bool = False

    def __post_init__(self):
        check_aggregate(self.aggregate, self.trim, self.clip_tau, self.clip_iters)


def check_aggregate(aggregate, trim, clip_tau=0.0, clip_iters=3):
    if aggregate not in AGGREGATES:
        raise ValueError(f"aggregate must be one of {AGGREGATES}, got {aggregate!r}")
    if not isinstance(trim, int) or trim < 0:
        raise ValueError(f"trim must be an integer >= 0, got {trim!r}")
    check_clip(clip_tau, clip_iters)


@dataclass
class StepStats:
    step: int
    loss: float | None
    synced: bool
    sync_ms: float = 0.0
    members: int = 1
    extra: dict = field(default_factory=dict)


class LocalSGDTrainer:
    def __init__(self, model: torch.nn.Module, cfg: LocalSGDConfig, *, group=None, membership=None,
                 device=None, compressor=None, tracer=None):
        self.model = model
        self.cfg = cfg
        self.device = device or next(model.parameters()).device
        self.flat = FlatParams(model, dtype=torch.bfloat16, device=self.device)
        self.buffers = FlatBuffers(model)  # BN running stats: averaged at every sync
        n = self.flat.numel
        self.master = self.flat.param.float()
        if cfg.opt_state not in ("fp32", "compact"):
            raise ValueError(f"opt_state must be 'fp32' or 'compact', got {cfg.opt_state!r}")
        # again: the config is mutable after its own check
        check_aggregate(cfg.aggregate, cfg.trim, cfg.clip_tau, cfg.clip_iters)
        # fault injection (tests, `train --byzantine`): called on self.delta after lsgd_delta, before the collective
        self.delta_hook = None
        # the same for the wire: called on this peer's own q8 records (uint8 [P, record]) after encode
        self.wire_hook = None
        self.trim_share = None  # robust rules: per rank, the share of its elements trimmed in the last round
        # robust rules over q8: the share of the coordinates whose aggregate was non-finite (more than `trim`
        # bad voters, or an overflowing sum; under cclip a non-finite centre) and came out as 0 in the last round
        self.nonfinite_share = None
        # cclip: per rank, its weight in the last round's last update (the mean over the shard owners); 1 = never
        # clipped, 0 = ignored. None under the other rules
        self.clip_weight = None
        self._trim_clip_logged = False
        self.cstate = None  # compact mode: the moments live here and self.m / self.v are None
        if cfg.opt_state == "compact":
            ops.check_compact_betas(cfg.betas)
            self.m = self.v = None
            self.cstate = ops.CompactState.zeros(n, self.device)
        else:
            self.m = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.v = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.anchor = self.master.clone()
        self.delta = torch.zeros(n, dtype=cfg.comm_dtype, device=self.device)
        self.outer_mom = torch.zeros(n, dtype=torch.float32, device=self.device) if cfg.outer_momentum > 0 else None
        self.ostate = ops.new_ostate(self.device, cfg.lr)
        # persistent partial buffers of the deferred column sums: never freed while the trainer lives (a captured
        # step keeps their addresses)
        self._colsums = ops.ColsumPool()
        self.membership = membership
        self.group = membership.group if membership is not None else group
        self.compressor = compressor
        self.tracer = tracer or NULL_TRACER  # utils/trace.py stage spans (HIP events)
        self.t = 0
        self.sync_count = 0
        self.last_sync_ms = 0.0
        self.t_sync_end = None
        self.failed_rounds = 0  # elastic rounds aborted mid-collective and redone
        self.admit_split = None  # the last admission transfer: communicator init vs broadcast (ms, bytes)
        self.last_round_stages = None  # a continuing member's stages of the last admission round
        # bench.py: time the averaging collective alone (device-synchronised on both sides) and
        # record its bytes, for algbw / busbw in the bench JSON
        self.time_reduce = False
        self.reduce_log: list[tuple[float, int]] = []  # (ms, bytes per rank) of each timed collective

    # ------------------------------------------------------------------ per step
    def set_lr(self, lr: float):
        self.ostate[1].fill_(lr)

    def forward_backward(self, x, y):
        self.flat.zero_grad()
        loss = self.model(x, y)
        # the bias / LayerNorm column sums of every layer are finished together on leaving the scope, before
        # grad_sumsq / clip / AdamW read the gradient (eager and captured step alike: capture() records this)
        with ops.deferred_colsums(self._colsums):
            loss.backward()
        return loss

    def optimizer_step(self):
        c = self.cfg
        kw = dict(n_decay=self.flat.n_decay, beta1=c.betas[0], beta2=c.betas[1], eps=c.eps, wd=c.weight_decay,
                  max_norm=c.max_grad_norm)
        if self.cstate is not None:
            ops.adamw_step_compact(self.flat.param, self.flat.grad, self.master, self.cstate, self.ostate, **kw)
        else:
            ops.adamw_step(self.flat.param, self.flat.grad, self.master, self.m, self.v, self.ostate, **kw)

    # ------------------------------------------------------------------ hipGraph capture
    def capture(self, x, y, warmup: int = 3):
        """Capture zero-grad + forward + backward + fused AdamW of one local step into a
        hipGraph (torch.cuda.graph). Replays then cost one graph launch instead of ~300
        kernel launches; the averaging round stays outside the graph (collective,
        membership). x/y shapes are fixed from here on. Runs `warmup` real steps first."""
        assert x.is_cuda, "graph capture needs GPU tensors"
        self.graph = None
        self._gx = x.clone()
        self._gy = y.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):  # real steps (eager; an H boundary still averages)
                self.step(self._gx, self._gy)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # thread_local: a process-group watchdog thread querying its events during capture
        # must not invalidate it
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            self._gloss = self.forward_backward(self._gx, self._gy)
            self.optimizer_step()
        self.graph = graph
        return self

    def step(self, x, y) -> StepStats:
        tr = self.tracer
        if getattr(self, "graph", None) is not None:
            if x.data_ptr() != self._gx.data_ptr():
                self._gx.copy_(x, non_blocking=True)
                self._gy.copy_(y, non_blocking=True)
            with tr.span("local_step_graph"):
                self.graph.replay()
            loss = self._gloss
        else:
            with tr.span("fwd_bwd"):
                loss = self.forward_backward(x, y)
            with tr.span("adamw"):
                self.optimizer_step()
        self.t += 1
        synced = False
        if self.t % self.cfg.H == 0:
            with tr.span("average"):
                self.sync()
            synced = True
        return StepStats(self.t, None, synced, self.last_sync_ms, self.group.size if self.group else 1,
                         {"loss_t": loss.detach()})

    # ------------------------------------------------------------------ averaging
    def sync(self):
        t0 = time.perf_counter()
        if self.membership is None:
            res = self._reduce(())
            self._apply(res)
            self.buffers.average_(self.group, self.cfg.aggregate, self.cfg.trim)
        else:
            self._sync_elastic()
        self.sync_count += 1
        self.last_sync_ms = (time.perf_counter() - t0) * 1e3
        self.t_sync_end = time.time()

    def _sync_elastic(self):
        """One elastic averaging round: agreed outcome -> guarded admission + reduction ->
        agreed verdict -> apply. A member dying inside the collectives aborts the round on
        every survivor; they restore the pre-round state (anchor/master were never touched,
        the pseudo-gradient is recomputed, the compressor state is rolled back) and redo the
        round on the next generation."""
        mem = self.membership
        t0 = time.perf_counter()
        grp, _, newcomers = mem.sync_round()
        t1 = time.perf_counter()
        self.last_round_stages = None
        while True:
            self.group = grp
            snap = self.compressor.snapshot() if (self.compressor is not None and grp.size > 1) else None
            try:
                with mem.guard():
                    t2 = time.perf_counter()
                    adopted = self._admit_newcomers(newcomers) if newcomers else None
                    self._dev_sync()
                    t3 = time.perf_counter()
                    res = self._reduce(newcomers)
                    bufs = self.buffers.averaged(grp, self.cfg.aggregate, self.cfg.trim, self._voters(grp, newcomers))
                    self._dev_sync()
                    t4 = time.perf_counter()
                self._adopt(adopted)  # nothing is applied before the verdict is `commit`
                self._apply(res, bufs)
                if newcomers:
                    # a continuing member's anatomy of an admission round (where the
                    # members' rejoin stall goes): membership agreement, the new group's first
                    # collective (RCCL communicator init), the model broadcast, the reduction, and
                    # what is left (guard entry / exit, verdict, apply)
                    self._dev_sync()
                    t5 = time.perf_counter()
                    ad = self.admit_split or {}
                    self.last_round_stages = {
                        "sync_round_ms": round((t1 - t0) * 1e3, 3),
                        "peer_wait_ms": round(ad.get("peer_wait_ms", 0.0), 3),
                        "comm_init_ms": round(ad.get("comm_init_ms", 0.0), 3),
                        "broadcast_ms": round(ad.get("broadcast_ms", 0.0), 3),
                        "reduce_ms": round((t4 - t3) * 1e3, 3),
                        "guard_verdict_apply_ms": round(((t5 - t1) - (t4 - t2)) * 1e3, 3),
                        "broadcast_bytes": ad.get("bytes", 0),
                    }
                return
            except PeerFailure:
                if snap is not None:
                    self.compressor.restore(snap)
                # an abandoned gloo op may still own the old pseudo-gradient buffer
                self.delta = torch.zeros_like(self.delta)
                self.failed_rounds += 1
                grp, _, newcomers = mem.recover()

    def _reduce(self, newcomers=()):
        """Pseudo-gradient + collective. Returns what `_apply` needs; touches no model state."""
        g = self.group
        c = self.cfg
        robust = c.aggregate != "mean"
        if robust:
            check_aggregate(c.aggregate, c.trim, c.clip_tau, c.clip_iters)
            clip_q8 = c.aggregate == "cclip" and c.cclip_q8 and isinstance(self.compressor, Quant8Compressor)
            if c.aggregate == "cclip" and self.compressor is not None and not clip_q8:
                raise ValueError(f"aggregate='cclip' cannot be combined with the {type(self.compressor).__name__} "
                                 "compressor: the rule measures every peer's l2 distance from the centre; top-k and "
                                 "PowerSGD never put the peers' own values on the shard owner, and over the q8 "
                                 "records the rule runs only on request: set LocalSGDConfig.cclip_q8 with a "
                                 "Quant8Compressor (the aggregate is then quantised again, and a non-finite "
                                 "coordinate comes out as 0 and is counted in nonfinite_share)")
            if self.compressor is not None and not isinstance(self.compressor, Quant8Compressor):
                raise ValueError(f"aggregate={c.aggregate!r} cannot be combined with the "
                                 f"{type(self.compressor).__name__} compressor: a coordinate-wise rule needs every "
                                 "peer's own value of every coordinate on the shard owner, and top-k sends a "
                                 "different set of coordinates from every peer while PowerSGD sums low-rank "
                                 "factors; q8 is the compressor that works with the robust rules")
            if self.compressor is not None and not c.robust_q8 and not clip_q8:
                raise ValueError(f"aggregate={c.aggregate!r} is combined with the q8 compressor only on request: set "
                                 "LocalSGDConfig.robust_q8 (the rule then runs on the peers' decoded 8-bit records: "
                                 "the aggregate is quantised again, and a non-finite coordinate comes out as 0 and "
                                 "is counted in nonfinite_share)")
            if c.algo != "direct":
                raise ValueError(f"aggregate={c.aggregate!r} runs over the 'direct' exchange only, got "
                                 f"algo={c.algo!r}")
        if g is None or g.size == 1:
            return None
        ops.lsgd_delta(self.master, self.anchor, self.delta)
        if self.delta_hook is not None:
            self.delta_hook(self.delta)
        if isinstance(self.compressor, Quant8Compressor):
            self.compressor.wire_hook = self.wire_hook
        if robust:
            return self._reduce_robust(g, newcomers)
        contributors = max(1, g.size - len(newcomers))  # newcomers hold delta == 0
        if self.compressor is not None:
            avg = self.compressor.allreduce_mean(self.delta, g)
            return avg, g.size / contributors
        with self._timed_reduce():
            allreduce_sum_(self.delta, g, self.cfg.algo)
        return self.delta, 1.0 / contributors

    @contextlib.contextmanager
    def _timed_reduce(self):
        """Under `time_reduce`: the collective inside, between two device synchronisations, goes into `reduce_log`."""
        if not self.time_reduce:
            yield
            return
        self._dev_sync()
        t0 = time.perf_counter()
        yield
        self._dev_sync()
        self.reduce_log.append(((time.perf_counter() - t0) * 1e3, self.delta.numel() * self.delta.element_size()))

    @staticmethod
    def _voters(g, newcomers):
        """Ranks of `g` that hold a trained model: everyone but the newcomers, whose all-zero
        pseudo-gradient (and untrained buffers) must not vote. None: all ranks."""
        if not newcomers:
            return None
        live = [i for i, m in enumerate(g.members) if m not in newcomers]
        return live or None  # nobody holds a model yet: every delta is zero, everyone may vote

    def _reduce_robust(self, g, newcomers):
        """The averaging round under a robust rule: the trimmed mean itself ends up in self.delta."""
        c = self.cfg
        live = self._voters(g, newcomers)
        K = g.size if live is None else len(live)
        if c.aggregate == "cclip" and self.compressor is not None:  # q8 with cclip_q8: anything else was refused
            avg, w, nonfinite = self.compressor.allreduce_cclip(self.delta, g, c.clip_tau, c.clip_iters, live)
            self.clip_weight = w.tolist()
            self.nonfinite_share = nonfinite / self.delta.numel()
            return avg, 1.0
        if c.aggregate == "cclip":
            with self._timed_reduce():
                w = cclip_mean_(self.delta, g, c.clip_tau, c.clip_iters, live)
            self.clip_weight = w.tolist()
            return self.delta, 1.0
        trim = effective_trim(c.aggregate, c.trim, K)
        if trim > (K - 1) // 2 and not self._trim_clip_logged:
            self._trim_clip_logged = True
            print(f"[local-sgd] trim={trim} clipped to {(K - 1) // 2}: only {K} peers vote "
                  f"(a trimmed mean needs K >= 2 trim + 1)", flush=True)
        if self.compressor is not None:  # q8 (anything else was refused): the trimmed mean of the decoded records
            avg, counts, nonfinite = self.compressor.allreduce_robust(self.delta, g, trim, live)
            self.trim_share = (counts.double() / self.delta.numel()).tolist()
            self.nonfinite_share = nonfinite / self.delta.numel()
            return avg, 1.0
        with self._timed_reduce():
            counts = robust_mean_(self.delta, g, trim, live)
        self.trim_share = (counts.double() / self.delta.numel()).tolist()
        return self.delta, 1.0

    def _apply(self, res, bufs=None):
        if bufs is not None:
            self.buffers.load_fp32(bufs)
        if res is None:
            self.anchor.copy_(self.master)
            return
        avg, scale = res
        c = self.cfg
        ops.lsgd_apply(avg, self.anchor, self.master, self.flat.param, self.outer_mom, outer_lr=c.outer_lr,
                       mu=c.outer_momentum, nesterov=c.nesterov, avg_scale=scale)

    def _average(self, newcomers=()):
        self._apply(self._reduce(newcomers))

    def _admit_newcomers(self, newcomers):
        """The generation contains peers without the model (joiners, or members whose earlier
        admission was aborted): the first continuing member broadcasts ONE packed fp32 vector
        [anchor | outer momentum | BN buffers] (identical on every continuing member) to the whole
        group, so every newcomer gets it in one pipelined collective instead of one point-to-point
        transfer per newcomer from the same root (RCCL: ring/tree broadcast over the xGMI links).
        Everyone receives into scratch; a newcomer adopts the model only after the round's verdict
        is `commit` (``_adopt``), so an aborted transfer can never corrupt any peer.
        Returns what the newcomer adopts (None on continuing members)."""
        g = self.group
        members = g.members
        cont = [i for i, m in enumerate(members) if m not in newcomers]
        if not cont:
            return None  # nobody holds a model yet: everyone starts from its own (identical) init
        root = cont[0]
        dev = self.anchor.device
        parts = [self.anchor] + ([self.outer_mom] if self.outer_mom is not None else [])
        nb = self.buffers.numel if self.buffers else 0
        n = sum(p.numel() for p in parts) + nb
        bdev = dev if g.backend == "nccl" else torch.device("cpu")
        if g.rank == root:
            pack = torch.cat([p.reshape(-1).to(bdev) for p in parts]
                             + ([self.buffers.as_fp32().to(bdev)] if nb else []))
        else:
            pack = torch.empty(n, dtype=torch.float32, device=bdev)
        # every member of the new group checks in at the rendezvous store first, so the communicator
        # set-up below is timed from the moment the LAST rank arrived: a member that enters the admission
        # round while a joiner is still starting up waits here (peer_wait_ms), not inside the init
        # (the members' 2.56 s vs the joiners' 1.34 s of "communicator init")
        tw = time.perf_counter()
        self._admission_checkin(g)
        # a one-element collective first: its time is the new group's communicator set-up (RCCL builds
        # its communicator lazily, at the first collective) plus one latency, so the broadcast time
        # below is the model transfer alone
        t0 = time.perf_counter()
        g.broadcast_(torch.zeros(1, dtype=torch.float32, device=bdev), root)
        self._dev_sync()
        t1 = time.perf_counter()
        g.broadcast_(pack, root)
        self._dev_sync()
        t2 = time.perf_counter()
        self.admit_split = {"peer_wait_ms": (t0 - tw) * 1e3, "comm_init_ms": (t1 - t0) * 1e3,
                            "broadcast_ms": (t2 - t1) * 1e3, "bytes": int(n * 4)}
        return pack if members[g.rank] in newcomers else None

    def _admission_checkin(self, g):
        """Store barrier of the admission round's group (elastic runs only): add one to the generation's
        check-in counter and wait until every member has; a trip of the watchdog (a member died) ends
        the wait as a PeerFailure like any guarded collective."""
        mem = self.membership
        if mem is None or g.size <= 1:
            return
        key = f"vcx/el/admit_in/{mem.gen}"
        mem.store.add(key, 1)
        while int(mem.store.add(key, 0)) < g.size:
            if mem.tripped():
                raise PeerFailure(f"gen {mem.gen}: aborted during the admission check-in ({mem.abort_reason()})")
            time.sleep(0.001)

    def _dev_sync(self):
        if self.anchor.is_cuda:
            torch.cuda.synchronize(self.anchor.device)

    def _adopt(self, pack):
        """A newcomer takes the admitted model (after `commit`)."""
        if pack is None:
            return
        pack = pack.to(self.anchor.device)
        n0 = self.anchor.numel()
        self.anchor.copy_(pack[:n0])
        pos = n0
        if self.outer_mom is not None:
            self.outer_mom.copy_(pack[pos:pos + n0])
            pos += n0
        if self.buffers:
            self.buffers.load_fp32(pack[pos:pos + self.buffers.numel])
        self.master.copy_(self.anchor)
        ops.f32_to_bf16(self.anchor, self.flat.param)

    def join_running_job(self):
        """Called by a peer that was just admitted (``membership.join()``): receive the model
        and take part in the round that admitted it (retried on the next generation if a
        member dies during it)."""
        mem = self.membership
        grp, newcomers = mem.group, mem.newcomers
        dev_sync = (lambda: torch.cuda.synchronize(self.anchor.device)) if self.anchor.is_cuda else (lambda: None)
        while True:
            self.group = grp
            try:
                # stage times of the admission (bench_drop.py reports them): communicator connect,
                # the wait for the members to enter the admission round (staged admission: they
                # finish their local steps first), then the round itself -- model broadcast,
                # reduction, verdict + apply
                t0 = time.perf_counter()
                with mem.guard():  # connect, then line up with the continuing members (wait_round_start)
                    dev_sync()
                    t2 = time.perf_counter()
                    t1 = t2 - mem.last_go_wait_ms * 1e-3
                    adopted = self._admit_newcomers(newcomers)
                    dev_sync()
                    t3 = time.perf_counter()
                    res = self._reduce(newcomers)
                    bufs = self.buffers.averaged(grp, self.cfg.aggregate, self.cfg.trim, self._voters(grp, newcomers))
                    dev_sync()
                    t4 = time.perf_counter()
                self._adopt(adopted)
                self._apply(res, bufs)
                dev_sync()
                t5 = time.perf_counter()
                ad = self.admit_split or {}
                st = {"connect_ms": (t1 - t0) * 1e3, "wait_round_ms": (t2 - t1) * 1e3,
                      "peer_wait_ms": ad.get("peer_wait_ms", 0.0), "comm_init_ms": ad.get("comm_init_ms", 0.0), "broadcast_ms": ad.get("broadcast_ms", (t3 - t2) * 1e3),
                      "reduce_ms": (t4 - t3) * 1e3,
                      "verdict_apply_ms": (t5 - t4) * 1e3, "admission_round_ms": (t5 - t2) * 1e3,
                      "broadcast_bytes": ad.get("bytes", int(self.anchor.numel() * 4 * (2 if self.outer_mom is not None else 1)))}
                self.admit_stages = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in st.items()}
                return
            except PeerFailure:
                self.delta = torch.zeros_like(self.delta)
                self.failed_rounds += 1
                grp, _, newcomers = mem.recover()

    # ------------------------------------------------------------------ state
    def state_tensors(self):
        if self.cstate is not None:
            moments = dict(zip(self.cstate.FIELDS, self.cstate.arrays()))
        else:
            moments = {"m": self.m, "v": self.v}
        return {"master": self.master, **moments, "anchor": self.anchor, "ostate": self.ostate}

    def checkpoint_slice(self):
        """This peer's 1/P share of the (synchronised) state: call right after a sync round,
        when master == anchor on every peer. Adam moments and the compressor's error feedback
        are per-peer; the checkpoint stores their mean over the peers (one reduce-scatter each,
        so every peer writes the averaged slice it owns) — a restore onto any peer count then
        starts every peer from the same coherent moments, and from the mean unsent residual
        (exactly what the next averaging round would have delivered)."""
        P = 1 if self.group is None else self.group.size
        r = 0 if self.group is None else self.group.rank
        lo, hi = self.flat.shard_bounds(r, P)
        # compact: the checkpoint holds fp32 moments either way, decoded before the mean over the peers
        m, v = self.cstate.to_fp32() if self.cstate is not None else (self.m, self.v)
        t = {"master": self.anchor[lo:hi], "m": mean_slice(self.group, m, lo, hi),
             "v": mean_slice(self.group, v, lo, hi)}
        if self.outer_mom is not None:
            t["outer_mom"] = self.outer_mom[lo:hi]  # identical on every peer (updated from the average)
        if self.compressor is not None:
            t["ef"] = mean_slice(self.group, self.compressor.state_dict()["ef"], lo, hi)
        return lo, hi, t

    def checkpoint_global(self) -> dict:
        """Tensors written once (by the writer peer) next to the parameters."""
        out = {}
        if self.buffers:
            out["buffers"] = self.buffers.as_fp32()
        if self.compressor is not None and "Q" in self.compressor.state_dict():
            out["psgd_Q"] = self.compressor.state_dict()["Q"]  # identical on every peer (all-reduced)
        return out

    def restore(self, reader):
        reader.check_layout(self.flat)
        n = self.flat.numel
        dev = self.device
        self.master.copy_(reader.read_range("master", 0, n).to(dev))
        self.anchor.copy_(self.master)
        m, v = reader.read_range("m", 0, n).to(dev), reader.read_range("v", 0, n).to(dev)
        if self.cstate is not None:
            self.cstate.load_fp32(m, v)
        else:
            self.m.copy_(m)
            self.v.copy_(v)
        if self.outer_mom is not None:
            self.outer_mom.copy_(reader.read_range("outer_mom", 0, n).to(dev))
        _, ost = reader.params()
        self.ostate.copy_(ost.to(dev))
        ops.f32_to_bf16(self.master, self.flat.param)
        restore_extras(self, reader)
        self.t = reader.step


def mean_slice(group, buf, lo, hi):
    """[lo, hi) of the peers' mean of `buf` (this peer's shard): one reduce-scatter."""
    if group is None or group.size == 1:
        return buf[lo:hi]
    P = group.size
    if buf.numel() % P == 0 and hi - lo == buf.numel() // P:
        out = torch.empty(hi - lo, dtype=buf.dtype, device=buf.device)
        group.reduce_scatter_(out, buf)
    else:
        tmp = buf.clone()
        group.allreduce_(tmp)
        out = tmp[lo:hi]
    return out.div_(P)


def restore_extras(trainer, reader):
    """BN buffers and compressor state (error feedback, PowerSGD's Q) if the checkpoint has them."""
    bufs = reader.global_tensor("buffers")
    if bufs is not None and trainer.buffers:
        trainer.buffers.load_fp32(bufs)
    comp = trainer.compressor
    if comp is not None and reader.has_key("ef"):
        d = {"ef": reader.read_range("ef", 0, trainer.flat.numel)}
        q = reader.global_tensor("psgd_Q")
        if q is not None:
            d["Q"] = q
        elif "Q" in comp.state_dict():
            d["Q"] = comp.state_dict()["Q"]
        comp.load_state_dict(d)
