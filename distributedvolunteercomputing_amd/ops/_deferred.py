"""Deferred finish of the backward's small column sums (bias and LayerNorm gradients).

The backward kernels of ``add_layernorm``, ``causal_attention(bias=...)`` and the fused MLP leave fp32 partial
rows whose column sums are the gradients of gamma, beta and the biases. Finished on the spot that is a pair of
latency-bound launches per call site (86 per GPT-2-small step). The partials stay as they are until the optimizer
reads the gradients, so inside ``deferred_colsums()`` each backward only registers a job -- partial rows, the
slot of the flat gradient buffer, accumulate, zero_src -- and one ``colsum_finish_many`` sums every job of the
pass in one stage-1 and one stage-2 launch per ``JOB_TABLE_CAP`` jobs, with the same summation order, so the
gradients are bit-identical to the immediate finish.

Partial buffers are persistent: call site k of a backward pass (the order of registration) owns one buffer,
allocated on the first pass and reused by every later one, so a captured graph keeps their addresses. They live
as long as the pool does (the trainer's lifetime; the same rule as ``GPT2._wt_bufs``).

A second backward pass that starts while jobs of an earlier one are pending (gradient accumulation inside one
scope) first finishes the pending jobs: their partial buffers are about to be overwritten.
"""
from __future__ import annotations

import contextlib

import torch

from .. import config
from ._lib import native

_ACTIVE: list = []  # the stack of active pools (the autograd thread of one backward at a time)


class ColsumPool:
    """The persistent partial buffers of one model's backward pass, and the jobs pending on them."""

    def __init__(self):
        self._bufs: list[torch.Tensor] = []  # by order of registration within one backward pass
        self._next = 0
        self._round_open = False
        self._jobs: list[tuple[torch.Tensor, torch.Tensor, bool, bool]] = []  # (part, out, accumulate, zero_src)
        self._outs: set[int] = set()
        self._stage: torch.Tensor | None = None
        self.launches = 0  # kernel launches of the last finish()

    # ---------------------------------------------------------------- buffers
    def _begin(self):
        """First registration of a backward pass: restart the call-site count; jobs an earlier pass left pending
        are finished first, because this pass writes the same partial buffers."""
        if self._round_open:
            return
        if self._jobs:
            self.finish()
        self._round_open = True
        self._next = 0

        def _end():
            self._round_open = False

        torch.autograd.Variable._execution_engine.queue_callback(_end)

    def partials(self, shape, device, zero: bool = False) -> torch.Tensor:
        """The fp32 buffer of the next call site of this backward pass (allocated on the first pass). zero: it is
        a zero-at-rest accumulation buffer (zeroed when made; its zero_src job leaves it zeroed again)."""
        self._begin()
        k = self._next
        self._next += 1
        shape = tuple(int(s) for s in shape)
        buf = self._bufs[k] if k < len(self._bufs) else None
        if buf is None or tuple(buf.shape) != shape or buf.device != device:
            # pending jobs hold their own reference to a buffer this replaces
            buf = (torch.zeros if zero else torch.empty)(shape, device=device, dtype=torch.float32)
            if k < len(self._bufs):
                self._bufs[k] = buf
            else:
                self._bufs.append(buf)
        return buf

    def nbytes(self) -> int:
        """Bytes of partial buffers held (the stage buffer not included)."""
        return sum(b.numel() * 4 for b in self._bufs)

    def stage_nbytes(self) -> int:
        return 0 if self._stage is None else self._stage.numel() * 4

    # ---------------------------------------------------------------- jobs
    def register(self, part: torch.Tensor, out: torch.Tensor, accumulate: bool = True, zero_src: bool = False):
        """out[C] (bf16, a view of the flat gradient buffer) (+)= column sums of part [P, C], at finish()."""
        self._begin()
        if out.data_ptr() in self._outs:
            self.finish()  # two jobs of one launch must not add into the same slot (a parameter used twice)
        self._outs.add(out.data_ptr())
        self._jobs.append((part, out, bool(accumulate), bool(zero_src)))

    def pending(self) -> int:
        return len(self._jobs)

    def finish(self) -> int:
        """Sum every pending job into its gradient slot; returns the kernel launches made."""
        jobs, self._jobs = self._jobs, []
        self._outs = set()
        self.launches = 0
        if not jobs:
            return 0
        C = native()
        # widest jobs last: a table's grid is sized by its widest job
        jobs.sort(key=lambda j: j[1].numel())
        need = C.colsum_finish_stage_floats([j[1].numel() for j in jobs])
        dev = jobs[0][0].device
        if self._stage is None or self._stage.numel() < need or self._stage.device != dev:
            self._stage = torch.empty(need, device=dev, dtype=torch.float32)
        self.launches = int(C.colsum_finish_many([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs],
                                                 [j[3] for j in jobs], self._stage))
        return self.launches


_DEFAULT = ColsumPool()


def active() -> ColsumPool | None:
    """The pool backward ops register with, or None (finish at once): inside a ``deferred_colsums()`` scope with
    ``config.colsum_defer`` on."""
    if _ACTIVE and config.get().colsum_defer:
        return _ACTIVE[-1]
    return None


@contextlib.contextmanager
def deferred_colsums(pool: ColsumPool | None = None):
    """Inside the scope the backward of add_layernorm, causal_attention(bias=...) and the fused MLP registers its
    column-sum finish with ``pool`` (default: a process-wide one) when the result goes into a preset flat gradient
    buffer; leaving the scope, or ``pool.finish()``, launches the finish of all of them together. A gradient that
    autograd expects as a return value is finished at once, as outside the scope."""
    pool = _DEFAULT if pool is None else pool
    _ACTIVE.append(pool)
    try:
        yield pool
    finally:
        _ACTIVE.pop()
        pool.finish()
