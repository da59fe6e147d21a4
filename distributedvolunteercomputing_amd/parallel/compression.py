"""Communication compression with error feedback for averaging rounds / gradient steps.

* ``TopKCompressor``   — exact global top-k of |g + e| (radix select on the GPU), sparse
  all-gather of (index, value) pairs, scatter-add into a dense buffer. The unsent remainder
  stays in the error-feedback buffer ``e`` (BASELINE.json config 3: "top-k sparsified
  gradients + error feedback").
* ``PowerSGDCompressor`` — rank-r PowerSGD (Vogels et al., 2019) with warm-started Q and
  error feedback over every matrix of a ``FlatParams`` layout; vectors go uncompressed
  (BASELINE.json config 5: "PowerSGD rank-4 compression").
* ``Quant8Compressor`` — 8-bit quantisation in blocks of 128 with one fp32 scale each and error
  feedback (1.03 B per element, any model, nothing to tune), moved like the ``direct``
  all-reduce: all-to-all of the codes, a fused dequantise-sum-requantise on the shard owner,
  all-gather of the averaged codes. It is the one compressor that combines with the robust rules
  (``allreduce_robust``): the shard owner holds every peer's record before anything is summed, so the
  sum becomes the coordinate-wise trimmed mean of ops/robust.py over the decoded records, or centered clipping
  of the decoded records (``allreduce_cclip``).

All expose ``allreduce_mean(buf_bf16, group) -> averaged bf16 buffer`` so they plug into
``LocalSGDTrainer`` (compressing the pseudo-gradient) and the sharded data-parallel trainer
(compressing gradients). GPU tensors use the HIP kernels of ``compress.hip``; CPU tensors
use the torch reference below (same math).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..ops import robust
from ..ops._lib import native, use_native
from .flat_params import FlatParams


class TopKCompressor:
    """Exact top-k with error feedback. One round on the GPU: ``topk_ef`` (accumulate + 2-pass
    radix select + compaction, compress.hip) writes the k (index, value) pairs straight into this
    peer's slot of a packed wire buffer ``[k int32 indices | k values]``; ONE all-gather moves
    every peer's block; ``scatter_add_packed`` accumulates them into a preallocated fp32 dense
    buffer, converted into a preallocated bf16 output. No per-round allocation, no host sync."""

    def __init__(self, numel: int, ratio: float, device, value_dtype=torch.bfloat16):
        self.n = int(numel)
        self.k = max(1, int(math.ceil(numel * ratio)))
        self.device = torch.device(device)
        self.value_dtype = value_dtype
        self.e = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        vwords = (self.k + 1) // 2 if value_dtype == torch.bfloat16 else self.k
        self.L = self.k + vwords  # int32 words per peer on the wire
        self.wire = torch.zeros(self.L, dtype=torch.int32, device=self.device)
        self.state = torch.zeros(8, dtype=torch.int32, device=self.device)
        self.state_init = torch.tensor([0, self.k, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=self.device)
        words = native().topk_hist_words() if self.device.type == "cuda" else 1
        self.hist = torch.zeros(words, dtype=torch.int32, device=self.device)
        self._gathered = {}  # P -> [P, L] all-gather target
        self.dense = None  # fp32 [n], allocated on first use
        self.out = None  # bf16 [n]
        self.bytes_sent = 0

    @property
    def ratio(self) -> float:
        return self.k / self.n

    @property
    def idx(self) -> torch.Tensor:
        return self.wire[: self.k]

    @property
    def val(self) -> torch.Tensor:
        return self.wire[self.k:].view(self.value_dtype)[: self.k]

    def compress(self, g: torch.Tensor):
        """(idx int32 [k], val [k]) of the k largest |g + e| (views of the wire buffer); e keeps
        the rest."""
        if use_native(g):
            self.state.copy_(self.state_init)
            self.wire.zero_()  # unfilled slots (fewer than k nonzero candidates) must read 0
            native().topk_ef(g.contiguous(), self.e, self.k, self.state, self.hist, self.idx, self.val)
            return self.idx, self.val
        self.e.add_(g.float())
        _, i = torch.topk(self.e.abs(), self.k, sorted=False)
        self.idx.copy_(i.to(torch.int32))
        self.val.copy_(self.e[i].to(self.value_dtype))
        self.e[i] = self.e[i] - self.val.float()  # wire-dtype rounding residual stays in e
        return self.idx, self.val

    # ------------------------------------------------------------------ state
    def snapshot(self) -> dict:
        """Pre-round state for an elastic round that may be aborted and redone."""
        return {"e": self.e.clone()}

    def restore(self, snap: dict):
        # fresh tensors: an abandoned (gloo) op of the aborted round may still hold the old ones
        self.e = snap["e"]
        self.wire = torch.zeros_like(self.wire)
        self._gathered = {}

    def state_dict(self) -> dict:
        return {"ef": self.e}

    def load_state_dict(self, d: dict):
        self.e.copy_(d["ef"].to(self.e.device))

    def allreduce_mean(self, g: torch.Tensor, group) -> torch.Tensor:
        self.compress(g)
        P = 1 if group is None else group.size
        if P > 1:
            allw = self._gathered.get(P)
            if allw is None:
                allw = self._gathered[P] = torch.empty(P, self.L, dtype=torch.int32, device=self.device)
            group.all_gather_(allw.view(-1), self.wire)  # indices and values in ONE collective
        else:
            allw = self.wire.view(1, -1)
        self.bytes_sent += self.L * 4
        if self.dense is None:
            self.dense = torch.empty(self.n, dtype=torch.float32, device=self.device)
            self.out = torch.empty(self.n, dtype=torch.bfloat16, device=self.device)
        self.dense.zero_()
        if use_native(self.dense):
            native().scatter_add_packed(allw, self.k, self.value_dtype == torch.bfloat16, 1.0 / P, self.dense)
        else:
            for p in range(P):
                w = allw[p]
                vals = w[self.k:].view(self.value_dtype)[: self.k].float()
                self.dense.index_add_(0, w[: self.k].long(), vals / P)
        self.out.copy_(self.dense)
        return self.out


_Q8_INV127 = float(np.float32(1.0) / np.float32(127.0))  # the fp32 constant 1.0f / 127.0f


def q8_quantise(v: torch.Tensor):
    """The q8 codec on fp32 blocks ``v [nblocks, 128]`` -> (codes int8 [nblocks, 128], scales fp32
    [nblocks]). This IS the definition the kernels of compress.hip match bit for bit: every product
    is one fp32 operation, the divide is correctly rounded, rounding is half to even, and a block
    whose maximum magnitude is below 2^-100 sends nothing (scale 0, codes 0)."""
    amax = v.abs().amax(dim=1)
    ok = amax >= 2.0 ** -100
    zero = torch.zeros_like(amax)
    scale = torch.where(ok, amax * _Q8_INV127, zero)
    # tensor / tensor: one correctly rounded divide (scalar / tensor is reciprocal-then-multiply)
    inv = torch.where(ok, torch.full_like(amax, 127.0) / amax, zero)
    q = torch.round(v * inv.unsqueeze(1)).clamp_(-127.0, 127.0)
    return q.to(torch.int8), scale


class Quant8Compressor:
    """8-bit block quantisation with error feedback: 1.03 B per element instead of bf16's 2, for any
    model, with nothing to tune. One round over P peers follows the ``direct`` all-reduce:
    ``encode`` (v = g + e quantised in blocks of 128 into P wire records, e = v - decoded) ->
    all-to-all of the records -> ``reduce`` on the shard owner (sum of the decoded records in rank
    order, times 1/P, quantised again into one record) -> all-gather of that record -> ``decode``
    into a bf16 buffer. The second quantisation has no error feedback: its residual is at most
    half a code unit of the averaged block and identical on every peer. ``allreduce_robust`` is the
    same round with ``reduce_robust`` in the middle: the trimmed mean over the peers' decoded records
    in place of their sum, plus one small all-reduce of the trimmed / non-finite counters; ``allreduce_cclip``
    has ``reduce_cclip`` there, centered clipping of the decoded records, and all-reduces the weights.

    Layout: the n elements are padded to L = ceil(n / (128 P)) 128 P (no padded copy is made: the
    kernels bounds-check), shard j is the elements [j m, (j + 1) m) with m = L / P, and its record
    is m int8 codes followed by m / 128 fp32 scales, carried as uint8. ``e`` has length n whatever
    P is, so a membership change needs no re-layout. Buffers are preallocated for the current P: no
    per-round allocation in steady state and no host sync on the GPU path. Non-finite gradients are
    not supported (as with the other compressors): an Inf or NaN stays in ``e`` for good."""

    BLOCK = 128

    def __init__(self, numel: int, device):
        self.n = int(numel)
        self.device = torch.device(device)
        self.e = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self._bufs = {}  # (P, name) -> uint8 buffer, see _buf
        self.out = None  # bf16 [n], allocated on first use
        self.bytes_sent = 0
        # fault injection (LocalSGDTrainer.wire_hook): called on this peer's own wire records
        # (uint8 [P, record]) at the end of every encode
        self.wire_hook = None

    @property
    def bytes_per_element(self) -> float:
        """Bytes of a record per element: one code and 1/128 of an fp32 scale."""
        return 1.0 + 4.0 / self.BLOCK

    def layout(self, P: int):
        """(L, m, record bytes) for P peers."""
        step = self.BLOCK * P
        L = (self.n + step - 1) // step * step
        m = L // P
        return L, m, m + m // 32

    def _buf(self, P: int, name: str) -> torch.Tensor:
        """The preallocated uint8 buffer `name` of the P-peer layout: ``wire`` / ``recv`` /
        ``gathered`` hold P records, ``record`` one. Allocated on first use (P = 1 needs only
        ``wire``). Only the current P's buffers are kept: a membership change drops the others
        (about 3 B per element), and the round after it allocates."""
        b = self._bufs.get((P, name))
        if b is None:
            for stale in [k for k in self._bufs if k[0] != P]:
                del self._bufs[stale]
            k = 1 if name == "record" else P
            b = self._bufs[(P, name)] = torch.zeros(k * self.layout(P)[2], dtype=torch.uint8, device=self.device)
        return b

    # ------------------------------------------------------------------ the three stages
    def encode(self, g: torch.Tensor, P: int) -> torch.Tensor:
        """v = g + e quantised into this peer's P wire records (uint8 [P * record]); e = v - decoded."""
        L, m, rec = self.layout(P)
        wire = self._buf(P, "wire")
        if use_native(g):
            native().q8_encode(g.contiguous(), self.e, L, P, wire)
            return self._hooked(wire, P)
        v = torch.zeros(L, dtype=torch.float32, device=g.device)
        v[: self.n] = self.e + g.float()
        q, scale = q8_quantise(v.view(-1, self.BLOCK))
        dec = q.float() * scale.unsqueeze(1)
        self.e.copy_((v - dec.view(-1))[: self.n])
        w = wire.view(P, rec)
        w[:, :m] = q.view(P, m).view(torch.uint8)
        w[:, m:] = scale.view(P, m // self.BLOCK).view(torch.uint8)
        return self._hooked(wire, P)

    def _hooked(self, wire: torch.Tensor, P: int) -> torch.Tensor:
        if self.wire_hook is not None:
            self.wire_hook(wire.view(P, -1))
        return wire

    @classmethod
    def _unpack(cls, records: torch.Tensor, P: int):
        """records uint8 [P * record] -> (codes fp32 [P, m / 128, 128], scales fp32 [P, m / 128, 1])."""
        w = records.view(P, -1)
        m = w.shape[1] * 32 // 33
        q = w[:, :m].contiguous().view(torch.int8).float().view(P, m // cls.BLOCK, cls.BLOCK)
        scale = w[:, m:].contiguous().view(torch.float32).view(P, m // cls.BLOCK, 1)
        return q, scale

    def reduce(self, recv: torch.Tensor, P: int) -> torch.Tensor:
        """recv: the P peers' records of this peer's shard, in rank order -> one record of their mean
        (fp32 sum in rank order, times 1/P, quantised by the same codec)."""
        L, m, rec = self.layout(P)
        record = self._buf(P, "record")
        avg = float(np.float32(1.0 / P))
        if use_native(recv):
            native().q8_reduce(recv, P, m, avg, record)
            return record
        q, scale = self._unpack(recv, P)
        acc = torch.zeros(m // self.BLOCK, self.BLOCK, dtype=torch.float32, device=recv.device)
        for p in range(P):
            acc = acc + q[p] * scale[p]
        acc = acc * avg
        q2, s2 = q8_quantise(acc)
        record[:m] = q2.view(-1).view(torch.uint8)
        record[m:] = s2.view(torch.uint8)
        return record

    def reduce_robust(self, recv: torch.Tensor, P: int, trim: int, live_mask: int | None, valid: int,
                      counts: torch.Tensor | None = None, nonfinite: torch.Tensor | None = None) -> torch.Tensor:
        """The robust sibling of ``reduce``: one record of the coordinate-wise trimmed mean
        (ops/robust.py) of the P peers' decoded records of this peer's shard. The definition, which
        the HIP kernel q8_trimmed_reduce matches bit for bit:

        * dec[p][i] = float(code) * scale, one fp32 multiply, on whatever bytes a peer sent: nothing
          is sanitised. A NaN product is taken as the canonical +NaN 0x7FC00000, because the sign and
          payload of a NaN that an operation produces differ between processors (0 * Inf is
          0xFFC00000 on x86, 0x7FC00000 on gfx950); a non-finite value is an extreme of the order
          either way and is trimmed first.
        * res, counts = trimmed_mean_reference(dec, f, live_mask) on fp32 rows.
        * a non-finite res[i] (more than f bad voters, or an overflowing sum) becomes +0 and adds 1
          to `nonfinite`: no update for that coordinate, and the round says so.
        * elements at or beyond `valid` (the padding beyond n) do not vote: result +0, no count.
        * res is quantised by the codec of the other stages (``q8_quantise``).

        `counts` (int64 [P]) and `nonfinite` (int64 [1]) are added to if given."""
        L, m, rec = self.layout(P)
        live_mask = robust.full_mask(P) if live_mask is None else int(live_mask)
        K, f, _ = robust.trim_plan(P, trim, live_mask)
        valid = int(valid)
        if not 0 <= valid <= m:
            raise ValueError(f"reduce_robust: valid must be in 0..{m}, got {valid}")
        if recv.dtype != torch.uint8 or recv.numel() < P * rec:
            raise ValueError(f"reduce_robust: recv must hold {P} uint8 records of {rec} bytes")
        for t, k, what in ((counts, P, "counts"), (nonfinite, 1, "nonfinite")):
            if t is not None and (t.dtype != torch.int64 or t.numel() != k):
                raise ValueError(f"reduce_robust: {what} must hold {k} int64")
        record = self._buf(P, "record")
        if use_native(recv):
            native().q8_trimmed_reduce(recv, P, m, f, live_mask, valid, record, counts, nonfinite)
            return record
        out, c, bad = self.reduce_robust_reference(recv, P, f, live_mask, valid)
        record.copy_(out)
        if counts is not None:
            counts.add_(c.to(counts.device))
        if nonfinite is not None:
            nonfinite.add_(bad.to(nonfinite.device))
        return record

    @classmethod
    def reduce_robust_reference(cls, recv: torch.Tensor, P: int, trim: int, live_mask: int, valid: int):
        """The definition of ``reduce_robust`` in torch, on recv's device whichever it is: (record uint8
        [rec], counts int64 [P], nonfinite int64 scalar) of the P records in `recv`."""
        rec = recv.numel() // P
        m = rec * 32 // 33
        q, scale = cls._unpack(recv[: P * rec], P)
        dec = (q * scale).view(P, m)[:, :valid]
        nan = torch.tensor([0x7FC00000], dtype=torch.int32, device=recv.device).view(torch.float32)
        dec = torch.where(torch.isnan(dec), nan, dec)
        res, c = robust.trimmed_mean_reference(dec, trim, live_mask)
        bad = ~torch.isfinite(res)
        out = torch.zeros(m, dtype=torch.float32, device=recv.device)
        out[:valid] = torch.where(bad, torch.zeros_like(res), res)
        q2, s2 = q8_quantise(out.view(-1, cls.BLOCK))
        return torch.cat([q2.view(-1).view(torch.uint8), s2.view(torch.uint8)]), c, bad.sum()

    def reduce_cclip(self, recv: torch.Tensor, P: int, live_mask: int | None, valid: int, tau: float, iters: int,
                     weights: torch.Tensor | None = None, nonfinite: torch.Tensor | None = None) -> torch.Tensor:
        """The per-peer sibling of ``reduce_robust``: one record of centered clipping (ops/robust.py) of the P
        peers' decoded records of this peer's shard. ``reduce_cclip_reference`` holds the definition; the HIP
        kernels (q8_cclip_*, compress.hip) match it bit for bit and run on GPU tensors, the reference elsewhere,
        with the same refusals. `weights` (fp32 [P]) receives the last update's weights, `nonfinite` (int64 [1])
        is added to, where given."""
        L, m, rec = self.layout(P)
        live_mask = robust.full_mask(P) if live_mask is None else int(live_mask)
        robust.cclip_plan(P, live_mask, tau, iters)
        valid = int(valid)
        if not 0 <= valid <= m:
            raise ValueError(f"reduce_cclip: valid must be in 0..{m}, got {valid}")
        if recv.dtype != torch.uint8 or recv.numel() < P * rec:
            raise ValueError(f"reduce_cclip: recv must hold {P} uint8 records of {rec} bytes")
        for t, k, dt, what in ((weights, P, torch.float32, "weights"), (nonfinite, 1, torch.int64, "nonfinite")):
            if t is not None and (t.dtype != dt or t.numel() != k or t.device != recv.device):
                raise ValueError(f"reduce_cclip: {what} must hold {k} {dt} on recv's device")
        record = self._buf(P, "record")
        if use_native(recv):
            native().q8_cclip_reduce(recv, P, m, live_mask, valid, float(tau), iters, record, weights, nonfinite)
            return record
        out, w, bad, _ = self.reduce_cclip_reference(recv[: P * rec], P, live_mask, valid, tau, iters)
        record.copy_(out)
        if weights is not None:
            weights.copy_(w)
        if nonfinite is not None:
            nonfinite.add_(bad)
        return record

    @classmethod
    def reduce_cclip_reference(cls, recv: torch.Tensor, P: int, live_mask: int, valid: int, tau: float, iters: int):
        """The definition of ``reduce_cclip`` in torch, on recv's device whichever it is. recv: uint8 [P * rec], the
        peers' records of this owner's shard of m elements. A composition of two definitions the project holds bit
        for bit:

        1. Decode, as ``reduce_robust_reference``: dec[p][i] = float(code) * scale, one fp32 multiply, on whatever
           bytes a peer sent; a NaN product is taken as the canonical 0x7FC00000. Only dec[:, :valid] takes part.
        2. Clip: res, w, info = ops.robust.centered_clip_reference(dec[:, :valid], live_mask, tau, iters), the
           fp32-row rule unchanged. So the start is the median rule on fp32 rows, held in fp32; the distances are
           summed in the documented 4096-chunk, 256-slot, pairwise-tree order over the `valid` elements; a row that
           sends a non-finite value where the centre is finite gets weight 0; a coordinate whose centre is
           non-finite stays frozen; with one voter that row is returned unchanged and its weight is 1.
        3. Finish, as ``reduce_robust_reference``: a non-finite res[i] becomes +0 and adds 1 to `nonfinite`;
           elements at or beyond `valid` are +0 and are not counted; the m values are quantised by ``q8_quantise``
           into one record.

        Returns (record uint8 [rec], w fp32 [P], nonfinite int64 scalar, info); info is that of step 2 plus
        "result", the fp32 vector [valid] before the finish.

        Two consequences. Elements beyond `valid` add +0 to every distance, and a distance never becomes -0 (it
        is a sum of squares started at +0), so the sum over the `valid` elements here and the sum over all m
        elements in a kernel are the same bits. And no NaN that arithmetic produces can reach an output: the
        decode's NaN is made canonical before it is ordered; a NaN made in an update belongs either to a frozen
        coordinate, whose update is discarded, or to a centre that overflowed, which the finish zeroes and counts
        whatever its pattern; a NaN in a distance makes it non-finite and the weight 0 whatever its pattern. So
        the sign and payload of such NaNs, which differ between x86 and gfx950, do not matter."""
        rec = recv.numel() // P
        m = rec * 32 // 33
        valid = int(valid)
        q, scale = cls._unpack(recv[: P * rec], P)
        dec = (q * scale).view(P, m)[:, :valid]
        nan = torch.tensor([0x7FC00000], dtype=torch.int32, device=recv.device).view(torch.float32)
        dec = torch.where(torch.isnan(dec), nan, dec)
        res, w, info = robust.centered_clip_reference(dec, live_mask, tau, iters)
        info = dict(info, result=res)
        bad = ~torch.isfinite(res)
        out = torch.zeros(m, dtype=torch.float32, device=recv.device)
        out[:valid] = torch.where(bad, torch.zeros_like(res), res)
        q2, s2 = q8_quantise(out.view(-1, cls.BLOCK))
        return torch.cat([q2.view(-1).view(torch.uint8), s2.view(torch.uint8)]), w, bad.sum(), info

    def decode_f32(self, records: torch.Tensor, P: int) -> torch.Tensor:
        """The decoded fp32 values of the P gathered records, before the bf16 output rounding
        (torch reference; the tests' view of what a round transmitted)."""
        q, scale = self._unpack(records, P)
        return (q * scale).view(-1)[: self.n]

    def decode(self, records: torch.Tensor, P: int) -> torch.Tensor:
        """records: the P gathered records -> the preallocated bf16 [n] output buffer."""
        L = self.layout(P)[0]
        if self.out is None:
            self.out = torch.empty(self.n, dtype=torch.bfloat16, device=self.device)
        if use_native(records):
            native().q8_decode(records, L, P, self.out)
        else:
            self.out.copy_(self.decode_f32(records, P))
        return self.out

    # ------------------------------------------------------------------ state
    def snapshot(self) -> dict:
        """Pre-round state for an elastic round that may be aborted and redone."""
        return {"e": self.e.clone()}

    def restore(self, snap: dict):
        # fresh tensors: an abandoned (gloo) op of the aborted round may still hold the old ones
        self.e = snap["e"]
        self._bufs = {}

    def state_dict(self) -> dict:
        return {"ef": self.e}

    def load_state_dict(self, d: dict):
        self.e.copy_(d["ef"].to(self.e.device))

    def allreduce_mean(self, g: torch.Tensor, group) -> torch.Tensor:
        P = 1 if group is None else group.size
        wire = self.encode(g, P)
        if P == 1:
            return self.decode(wire, 1)
        recv, record, gathered = self._buf(P, "recv"), self._buf(P, "record"), self._buf(P, "gathered")
        rec = record.numel()
        group.alltoall_(recv, wire, [rec] * P, [rec] * P)
        self.reduce(recv, P)
        group.all_gather_(gathered, record)
        self.bytes_sent += 2 * (P - 1) * rec  # (P-1)/P of L + L/32 bytes out in each collective
        return self.decode(gathered, P)

    def allreduce_robust(self, g: torch.Tensor, group, trim: int, live_ranks=None):
        """``allreduce_mean`` with the trimmed mean of ``reduce_robust`` as the middle step: encode ->
        all-to-all -> reduce_robust -> all-gather -> all-reduce of the counters -> decode. `live_ranks`:
        the ranks that vote (default all); the others send their records and receive the result like
        everyone. Returns (avg bf16 [n], counts int64 [P], nonfinite int), the counters summed over
        the whole buffer and identical on every rank: per rank, the elements at which it was trimmed,
        and the coordinates whose aggregate was non-finite and came out as 0."""
        P, r = (1, 0) if group is None else (group.size, group.rank)
        mask = robust.mask_of(live_ranks, P)
        robust.trim_plan(P, trim, mask)  # every refusal before e is touched
        L, m, rec = self.layout(P)
        valid = min(max(self.n - r * m, 0), m)
        wire = self.encode(g, P)
        ctr = torch.zeros(P + 1, dtype=torch.int64, device=self.device)  # counts [P], then nonfinite
        if P == 1:
            gathered = self.reduce_robust(wire, 1, trim, mask, valid, ctr[:1], ctr[1:])
        else:
            recv, gathered = self._buf(P, "recv"), self._buf(P, "gathered")
            group.alltoall_(recv, wire, [rec] * P, [rec] * P)
            record = self.reduce_robust(recv, P, trim, mask, valid, ctr[:P], ctr[P:])
            group.all_gather_(gathered, record)
            ctr = ctr.to(group.device if group.backend == "nccl" else "cpu")
            group.allreduce_(ctr)
            self.bytes_sent += 2 * (P - 1) * rec + ctr.numel() * ctr.element_size()
        return self.decode(gathered, P), ctr[:P], int(ctr[P])

    def allreduce_cclip(self, g: torch.Tensor, group, tau: float, iters: int, live_ranks=None):
        """``allreduce_robust`` with centered clipping (``reduce_cclip``) as the middle step: encode -> all-to-all
        -> reduce_cclip -> all-gather -> one small all-reduce of the weights and the non-finite count -> decode.
        `live_ranks`: the ranks that vote (default all). Returns (avg bf16 [n], weights fp32 [P], nonfinite int),
        identical on every rank: per rank, the mean over the P shard owners of its last-update weight (as
        collectives.cclip_mean_), and the coordinates whose aggregate was non-finite and came out as 0."""
        P, r = (1, 0) if group is None else (group.size, group.rank)
        mask = robust.mask_of(live_ranks, P)
        robust.cclip_plan(P, mask, tau, iters)  # every refusal before e is touched
        L, m, rec = self.layout(P)
        valid = min(max(self.n - r * m, 0), m)
        wire = self.encode(g, P)
        w = torch.zeros(P, dtype=torch.float32, device=self.device)
        bad = torch.zeros(1, dtype=torch.int64, device=self.device)
        if P == 1:
            gathered = self.reduce_cclip(wire, 1, mask, valid, tau, iters, w, bad)
            return self.decode(gathered, 1), w, int(bad)
        recv, gathered = self._buf(P, "recv"), self._buf(P, "gathered")
        group.alltoall_(recv, wire, [rec] * P, [rec] * P)
        record = self.reduce_cclip(recv, P, mask, valid, tau, iters, w, bad)
        group.all_gather_(gathered, record)
        # one collective for both: fp64 holds the fp32 weights and a count below 2^53 exactly
        side = torch.cat([w.double(), bad.double()]).to(group.device if group.backend == "nccl" else "cpu")
        group.allreduce_(side)
        self.bytes_sent += 2 * (P - 1) * rec + side.numel() * side.element_size()
        return self.decode(gathered, P), (side[:P] / P).float(), int(side[P])


class PowerSGDCompressor:
    DESC_BYTES = 40  # sizeof(MatDesc) in compress.hip

    def __init__(self, flat: FlatParams, rank: int = 4, device=None, seed: int = 0, min_ratio: float = 2.0):
        assert rank in (1, 2, 4, 8), "rank must be 1, 2, 4 or 8"
        self.flat = flat
        self.rank = rank
        self.device = torch.device(device or flat.param.device)
        self.mats = []  # (offset, rows, cols)
        for s in flat.segments:
            if len(s.shape) < 2:
                continue
            rows = s.shape[0]
            cols = s.numel // rows
            if rows * cols < min_ratio * rank * (rows + cols):
                continue  # not worth compressing: sent dense
            self.mats.append((s.offset, rows, cols))
        self.dense_ranges = self._dense_ranges()
        R = rank
        self.p_off, self.q_off = [], []
        pt = qt = 0
        for off, r, c in self.mats:
            self.p_off.append(pt)
            self.q_off.append(qt)
            pt += r * R
            qt += c * R
        self.P = torch.zeros(max(pt, 1), dtype=torch.float32, device=self.device)
        g = torch.Generator().manual_seed(seed)  # identical warm-start Q on every peer
        self.Q = torch.randn(max(qt, 1), generator=g).to(self.device)
        self.e = torch.zeros(flat.numel, dtype=torch.float32, device=self.device)
        self.out = torch.zeros(flat.numel, dtype=torch.bfloat16, device=self.device)
        self.bytes_sent = 0
        # lazy error feedback (HIP path): reconstruct writes only the output and leaves the matrices
        # of `e` holding M = e_true + P Q^T; the next psgd_mq subtracts P Q^T in its own pass over M.
        # `ef()` returns the materialised error-feedback buffer.
        self._lazy_pending = False
        if self.device.type == "cuda":
            self._build_desc()

    def _dense_ranges(self):
        covered = np.zeros(0)
        ranges = []
        mats = sorted(self.mats)
        pos = 0
        for off, r, c in mats:
            if off > pos:
                ranges.append((pos, off))
            pos = off + r * c
        if pos < self.flat.numel:
            ranges.append((pos, self.flat.numel))
        del covered
        return ranges

    def _build_desc(self):
        def table(blocks_of):
            recs = np.zeros(len(self.mats), dtype=np.dtype([("off", "<i8"), ("poff", "<i8"), ("qoff", "<i8"),
                                                            ("rows", "<i4"), ("cols", "<i4"), ("blk0", "<i4"),
                                                            ("pad", "<i4")]))
            b = 0
            for i, (off, r, c) in enumerate(self.mats):
                recs[i] = (off, self.p_off[i], self.q_off[i], r, c, b, 0)
                b += blocks_of(r, c)
            return torch.from_numpy(recs.view(np.uint8).copy()).to(self.device), b

        C = native()
        rb, mr, mc = C.psgd_rows_per_block(), C.psgd_mtp_rows(), C.psgd_mtp_cols()
        self.d_mq, self.nb_mq = table(lambda r, c: (r + rb - 1) // rb)
        self.d_mtp, self.nb_mtp = table(lambda r, c: ((r + mr - 1) // mr) * ((c + mc - 1) // mc))
        self.d_rec = self.d_mq  # same row-block numbering
        self.nb_rec = self.nb_mq
        orows = C.psgd_orth_rows()
        self.d_orth, self.nb_orth = table(lambda r, c: (r + orows - 1) // orows)
        self.G = torch.zeros(2 * max(1, len(self.mats)) * self.rank * self.rank, dtype=torch.float32,
                             device=self.device)

    @property
    def compression_ratio(self) -> float:
        dense = sum(b - a for a, b in self.dense_ranges)
        sent = self.P.numel() + self.Q.numel() + dense
        return self.flat.numel / max(1, sent)

    def allreduce_mean(self, g: torch.Tensor, group) -> torch.Tensor:
        Pn = 1 if group is None else group.size
        nm = len(self.mats)
        R = self.rank
        native_path = use_native(g)
        if native_path:
            # the error-feedback accumulation e += g of the matrices runs inside psgd_mq (one pass
            # over e instead of two); the dense ranges accumulate in the loop at the end
            C = native()
        else:
            self.e.add_(g.float())
        if nm:
            if native_path:
                C.psgd_mq(self.d_mq, nm, self.nb_mq, self.e, self.Q, self.P, R, g, self._lazy_pending)
            else:
                self._materialise()
                self._ref_mq()
            if Pn > 1:
                group.allreduce_(self.P)
                self.P.div_(Pn)
            if native_path:
                C.psgd_orth(self.d_orth, nm, self.nb_orth, self.P, self.G, R)
            else:
                self._ref_orth()
            self.Q.zero_()
            if native_path:
                C.psgd_mtp(self.d_mtp, nm, self.nb_mtp, self.e, self.P, self.Q, R)
            else:
                self._ref_mtp()
            if Pn > 1:
                group.allreduce_(self.Q)
                self.Q.div_(Pn)
            if native_path:
                C.psgd_reconstruct(self.d_rec, nm, self.nb_rec, self.e, self.P, self.Q, self.out, R, False)
                self._lazy_pending = True
            else:
                self._ref_reconstruct()
                self._lazy_pending = False
        # vectors / small matrices: plain average, no error feedback needed
        for a, b in self.dense_ranges:
            seg = self.e[a:b]
            if native_path:
                seg.add_(g[a:b])
            if Pn > 1:
                group.allreduce_(seg)
                seg.div_(Pn)
            self.out[a:b].copy_(seg.to(torch.bfloat16))
            seg.zero_()
        self.bytes_sent += 4 * (self.P.numel() + self.Q.numel() + sum(b - a for a, b in self.dense_ranges))
        return self.out

    # ------------------------------------------------------------------ state
    def snapshot(self) -> dict:
        """Pre-round state for an elastic round that may be aborted and redone."""
        return {"e": self.e.clone(), "P": self.P.clone(), "Q": self.Q.clone(), "lazy": self._lazy_pending}

    def restore(self, snap: dict):
        # fresh tensors: an abandoned (gloo) op of the aborted round may still hold the old ones
        self.e, self.P, self.Q = snap["e"], snap["P"], snap["Q"]
        self._lazy_pending = snap["lazy"]
        self.out = torch.zeros_like(self.out)

    def state_dict(self) -> dict:
        """Error feedback (materialised: the pending lazy P Q^T subtracted) and the warm-start Q."""
        return {"ef": self.ef(), "Q": self.Q}

    def load_state_dict(self, d: dict):
        self.e.copy_(d["ef"].to(self.e.device))
        self.Q.copy_(d["Q"].to(self.Q.device))
        self._lazy_pending = False

    def _approx_sub(self, e):
        for i in range(len(self.mats)):
            off, r, c = self.mats[i]
            _, P, Q = self._views(i)
            e[off : off + r * c].view(r, c).sub_(P @ Q.t())

    def ef(self) -> torch.Tensor:
        """The error-feedback buffer e (a copy with the pending P Q^T subtracted if lazy)."""
        if not self._lazy_pending:
            return self.e
        e = self.e.clone()
        self._approx_sub(e)
        return e

    def _materialise(self):
        if self._lazy_pending:
            self._approx_sub(self.e)
            self._lazy_pending = False

    # ------------------------------------------------------------------ torch reference
    def _views(self, i):
        off, r, c = self.mats[i]
        R = self.rank
        M = self.e[off : off + r * c].view(r, c)
        P = self.P[self.p_off[i] : self.p_off[i] + r * R].view(r, R)
        Q = self.Q[self.q_off[i] : self.q_off[i] + c * R].view(c, R)
        return M, P, Q

    def _ref_mq(self):
        for i in range(len(self.mats)):
            M, P, Q = self._views(i)
            P.copy_(M @ Q)

    def _ref_orth(self):
        for i in range(len(self.mats)):
            _, P, _ = self._views(i)
            for a in range(self.rank):
                for b in range(a):
                    P[:, a] -= (P[:, a] @ P[:, b]) * P[:, b]
                P[:, a] /= P[:, a].norm() + 1e-8

    def _ref_mtp(self):
        for i in range(len(self.mats)):
            M, P, Q = self._views(i)
            Q.copy_(M.t() @ P)

    def _ref_reconstruct(self):
        for i in range(len(self.mats)):
            off, r, c = self.mats[i]
            M, P, Q = self._views(i)
            approx = P @ Q.t()
            M.sub_(approx)
            self.out[off : off + r * c].copy_(approx.reshape(-1).to(torch.bfloat16))
