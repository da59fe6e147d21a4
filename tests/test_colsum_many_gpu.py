"""The deferred finish of the backward's column sums (ops/_deferred.py, colsum_finish_many in norm_act.hip).

colsum_stage1_many / colsum_stage2_many run the bodies of the single-job kernels, so every job's result must be the
single-job path's (colsum_f32) bit for bit, whatever else shares its table. In a model the LayerNorm and QKV-bias
gradients are sums of partial rows the backward kernels write without atomics: deferred or not they are the same
bits. The fused MLP's fc-bias gradient is the bf16 rounding of an fp32 row that gemm_ps's epilogue sums with
atomics, so two runs of ONE path may differ in its last bit; the deferred path is held to the spread that runs of
the immediate path show among themselves (in bf16 ulps, measured here, no constant)."""
import importlib
import itertools

import pytest
import torch

from distributedvolunteercomputing_amd import config, ops
from distributedvolunteercomputing_amd.models.gpt2 import GPT2, GPT2Config
from distributedvolunteercomputing_amd.ops import _deferred
from distributedvolunteercomputing_amd.parallel.flat_params import FlatParams
from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer

pytestmark = pytest.mark.gpu

LIN = importlib.import_module("distributedvolunteercomputing_amd.ops.linear")  # the module, not ops.linear()

PS = (1, 5, 37, 256, 513)  # below one row per stage-1 chunk (32), not a multiple of 4 / 16 / 32
CS = (8, 72, 768, 3072)  # below 64, not a multiple of 64, the model widths
SHAPES = [(p, c, acc) for p, c in itertools.product(PS, CS) for acc in (False, True)]


def _jobs(n, gpu, seed=0):
    """n jobs cycling through every (P, C, accumulate), every third one zero_src: (parts, outs, acc, zero, want)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    C = ops.native()
    parts, outs, accs, zeros, want = [], [], [], [], []
    for k in range(n):
        P, Cw, acc = SHAPES[(k * 7) % len(SHAPES)]  # 7 is coprime to 40: neighbours in a table differ in C
        part = torch.randn(P, Cw, generator=g).to(gpu)
        out = torch.randn(Cw, generator=g).to(device=gpu, dtype=torch.bfloat16)
        want.append(C.colsum_f32(part.clone(), out.clone() if acc else None))
        parts.append(part)
        outs.append(out)
        accs.append(acc)
        zeros.append(k % 3 == 0)
    return parts, outs, accs, zeros, want


@pytest.mark.parametrize("n", [1, len(SHAPES), 64, 65, 130])
def test_many_matches_single_job_bitwise(gpu, n):
    """1, 40 (every P x C x accumulate in ONE table), 64, 65 and 130 jobs (the table split at 64)."""
    C = ops.native()
    parts, outs, accs, zeros, want = _jobs(n, gpu, seed=n)
    stage = torch.empty(C.colsum_finish_stage_floats([o.numel() for o in outs]), device=gpu)
    launches = C.colsum_finish_many(parts, outs, accs, zeros, stage)
    assert launches == 2 * ((n + C.JOB_TABLE_CAP - 1) // C.JOB_TABLE_CAP)
    for k in range(n):
        assert torch.equal(outs[k], want[k]), (k, SHAPES[(k * 7) % len(SHAPES)])
        if zeros[k]:
            assert int(torch.count_nonzero(parts[k])) == 0, k
        else:
            assert int(torch.count_nonzero(parts[k])) > 0, k


def test_one_row_zero_src_job_is_add_f32_into_bf16(gpu):
    """The fc-bias case: a one-row zero_src accumulate job does what add_f32_into_bf16(cs, gb, True, True) does."""
    C = ops.native()
    g = torch.Generator(device="cpu").manual_seed(4)
    for n in (8, 72, 3072):
        cs = torch.randn(n, generator=g).to(gpu)
        gb = torch.randn(n, generator=g).to(device=gpu, dtype=torch.bfloat16)
        cs2, want = cs.clone(), gb.clone()
        C.add_f32_into_bf16(cs2, want, True, True)
        stage = torch.empty(C.colsum_finish_stage_floats([n]), device=gpu)
        C.colsum_finish_many([cs], [gb], [True], [True], stage)
        assert torch.equal(gb, want) and int(torch.count_nonzero(cs)) == 0


def test_refusals(gpu):
    C = ops.native()
    part = torch.zeros(4, 64, device=gpu)
    out = torch.zeros(64, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="stage too small"):
        C.colsum_finish_many([part], [out], [False], [False], torch.empty(64, device=gpu))
    with pytest.raises(RuntimeError):
        C.colsum_finish_many([part], [out[:32]], [False], [False], torch.empty(1 << 16, device=gpu))
    x = torch.zeros(8, 128, device=gpu, dtype=torch.bfloat16)
    w = torch.ones(128, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="defer needs"):
        C.ln_bwd(x, x, w, torch.zeros(8, device=gpu), torch.ones(8, device=gpu), None, False, False, False, w.clone(),
                 None, None, None, True)


# ---------------------------------------------------------------- in a model
B, T = 2, 128
MODELS = {
    # the issue's block: C = 128, 2 heads of 64 (the attention-bias path), T = 128, B = 2
    "tiny": dict(vocab_size=512, padded_vocab=512, n_ctx=T, n_layer=1, n_head=2, n_embd=128),
    # the smallest width the fused MLP (gemm_ps) takes: its fc-bias gradients are the one-row zero_src jobs
    "w256": dict(vocab_size=512, padded_vocab=512, n_ctx=T, n_layer=2, n_head=4, n_embd=256),
}


def _model(gpu, name, seed=11):
    model = GPT2(GPT2Config(**MODELS[name]))
    model.reset_parameters(seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:  # biases and gains away from their 0 / 1 initial values
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return model.to(device=gpu, dtype=torch.bfloat16)


def _batch(gpu, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randint(0, 512, (B, T + 1), generator=g).to(gpu)
    return t[:, :-1].contiguous(), t[:, 1:].contiguous()


def _ulps(a, b):
    """The largest elementwise distance of two bf16 tensors in ulps of the larger magnitude."""
    a, b = a.float(), b.float()
    m = torch.maximum(a.abs(), b.abs())
    e = torch.frexp(m)[1].float()  # m = f * 2^e, f in [0.5, 1): one bf16 ulp of m is 2^(e - 8)
    d = (a - b).abs() / torch.exp2(e - 8)
    return float(torch.where(m > 0, d, torch.zeros_like(d)).max())


def _exact(name):
    """Sums of partial rows written without atomics: every LayerNorm gain / bias, the QKV and branch biases."""
    return ".ln" in name or name.startswith("lnf") or name.endswith((".attn_b", ".proj_b", ".fc2_b"))


def _assert_grads(got, offs, names):
    """got: the deferred run's gradients; offs: those of several immediate runs."""
    want = offs[0]
    n_exact = 0
    for n in names:
        if n.endswith(".fc_b"):
            spread = max(_ulps(x[n], y[n]) for x, y in itertools.combinations(offs, 2))
            dist = min(_ulps(got[n], o[n]) for o in offs)
            print(f"{n}: deferred-to-immediate {dist} ulp, immediate-to-immediate spread {spread} ulp")
            assert dist <= spread, (n, dist, spread)
        elif _exact(n):
            n_exact += 1
            assert torch.equal(got[n], want[n]), (n, float((got[n].float() - want[n].float()).abs().max()))
    return n_exact


@pytest.mark.parametrize("name", list(MODELS))
def test_model_backward_deferred_matches_immediate(gpu, name):
    model = _model(gpu, name)
    flat = FlatParams(model, device=gpu)
    x, y = _batch(gpu)
    pool = ops.ColsumPool()

    def run(defer):
        with config.override(colsum_defer=defer):
            flat.zero_grad()
            loss = model(x, y)
            with ops.deferred_colsums(pool):
                loss.backward()
                pending = pool.pending()
        return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, pending

    offs = [run(False) for _ in range(4)]
    assert all(o[2] == 0 for o in offs) and pool.nbytes() == 0
    got = run(True)
    L = MODELS[name]["n_layer"]
    b0 = model.blocks[0]
    fused = LIN._mlp_mode(torch.empty(B, T, b0.fc_w.shape[1], device=gpu, dtype=torch.bfloat16), b0.fc_w, b0.fc2_w) == "ps"
    assert fused or name != "w256"
    # per block 3 + 3 LayerNorm outputs (the first LayerNorm has no branch bias) and the QKV bias, the final
    # LayerNorm's 3 - 1 + ... : 2 + 3 * 2 * L LayerNorm jobs, L attention jobs, L fc-bias jobs on the fused MLP
    assert got[2] == 2 + 6 * L + L + (L if fused else 0), got[2]
    assert pool.pending() == 0 and pool.launches == 2
    assert torch.equal(got[0], offs[0][0])
    names = [n for n, _ in model.named_parameters()]
    n_exact = _assert_grads(got[1], [o[1] for o in offs], names)
    assert n_exact == 2 + 7 * L  # every LayerNorm gain / bias, proj_b, fc2_b and attn_b
    # a second deferred pass reuses the persistent buffers and gives the same bits
    ptrs, held = [b.data_ptr() for b in pool._bufs], pool.nbytes()
    again = run(True)
    assert [b.data_ptr() for b in pool._bufs] == ptrs and pool.nbytes() == held
    _assert_grads(again[1], [o[1] for o in offs], names)


def test_second_backward_finishes_the_pending_jobs_first(gpu):
    """Two backward passes inside ONE scope (gradient accumulation): the second pass writes the partial buffers the
    first one's pending jobs point at, so its first registration finishes them; the sum of both passes is the
    immediate path's. On a LayerNorm + fused MLP chain with the model's parameters and flat gradient buffers."""
    model = _model(gpu, "w256")
    flat = FlatParams(model, device=gpu)
    b0 = model.blocks[0]
    g = torch.Generator(device="cpu").manual_seed(9)
    h = torch.randn(B * T, 256, generator=g).to(device=gpu, dtype=torch.bfloat16)
    dy = torch.randn(B * T, 256, generator=g).to(device=gpu, dtype=torch.bfloat16)
    names = {"blocks.0.ln2_w": b0.ln2_w, "blocks.0.ln2_b": b0.ln2_b, "blocks.0.fc_b": b0.fc_b}
    pool = ops.ColsumPool()
    seen = []

    def run(defer, passes):
        flat.zero_grad()
        with config.override(colsum_defer=defer):
            hn, _ = ops.add_layernorm(h, None, b0.ln2_w, b0.ln2_b)
            out = ops.mlp_gelu(hn, b0.fc_w, b0.fc_b, b0.fc2_w)
            loss = (out.float() * dy.float()).sum()
            with ops.deferred_colsums(pool):
                for i in range(passes):
                    loss.backward(retain_graph=i + 1 < passes)
                    seen.append((defer, i, pool.pending(), {n: p.grad.detach().clone() for n, p in names.items()}))
        return {n: p.grad.detach().clone() for n, p in names.items()}

    offs = [run(False, 2) for _ in range(4)]
    once = run(True, 1)
    del seen[:]
    got = run(True, 2)
    # after either pass 3 jobs are pending (gain, bias, fc bias): the first pass's were finished when the second
    # began, so after the second pass the buffer holds exactly one pass's gradient (the second's are still pending)
    assert [(s[1], s[2]) for s in seen] == [(0, 3), (1, 3)]
    assert int(torch.count_nonzero(seen[0][3]["blocks.0.ln2_w"])) == 0  # nothing finished yet after the first pass
    assert torch.equal(seen[1][3]["blocks.0.ln2_w"], once["blocks.0.ln2_w"])
    assert pool.pending() == 0
    _assert_grads(got, offs, list(names))
    assert torch.equal(got["blocks.0.ln2_b"], offs[0]["blocks.0.ln2_b"])
    assert not torch.equal(got["blocks.0.ln2_w"], once["blocks.0.ln2_w"])  # the second pass did accumulate


@pytest.mark.parametrize("name", list(MODELS))
def test_captured_step_replays_equal_the_eager_step(gpu, name):
    """The captured step (trainer.capture: the finish is part of the graph, on the pool's persistent buffers)
    replayed twice against the eager step. With lr = 0 the weights stay put, so every step computes the same
    gradient: the loss and the exact gradients must be the eager step's bits after each replay, and the eager
    deferred step's those of the eager immediate step."""
    x, y = _batch(gpu)
    cfg = dict(H=100, lr=0.0, weight_decay=0.0)
    names = None

    def grads(tr):
        out = {}
        for s in tr.flat.segments:
            out[s.name] = tr.flat.grad[s.offset:s.offset + s.numel].detach().clone()
        return out

    def eager(defer):
        with config.override(colsum_defer=defer):
            tr = LocalSGDTrainer(_model(gpu, name), LocalSGDConfig(**cfg), device=gpu)
            st = tr.step(x, y)
            torch.cuda.synchronize()
            return st.extra["loss_t"].detach().clone(), grads(tr), tr

    offs = [eager(False) for _ in range(4)]
    on = eager(True)
    names = list(on[1])
    assert on[2]._colsums.nbytes() > 0 and offs[0][2]._colsums.nbytes() == 0
    assert torch.equal(on[0], offs[0][0])
    n_exact = _assert_grads(on[1], [o[1] for o in offs], names)
    assert n_exact == 2 + 7 * MODELS[name]["n_layer"]
    tg = LocalSGDTrainer(_model(gpu, name), LocalSGDConfig(**cfg), device=gpu).capture(x, y, warmup=1)
    ptrs = [b.data_ptr() for b in tg._colsums._bufs]
    for _ in range(2):
        st = tg.step(x, y)
        torch.cuda.synchronize()
        assert torch.equal(st.extra["loss_t"], on[0])
        _assert_grads(grads(tg), [o[1] for o in offs], names)
    assert [b.data_ptr() for b in tg._colsums._bufs] == ptrs and tg._colsums.pending() == 0
    assert torch.equal(tg.master, on[2].master)  # lr = 0: nothing moved


def test_scope_off_and_gradients_returned_to_autograd(gpu):
    """Outside a scope, and for gradients autograd expects as return values (no preset flat buffer), nothing is
    deferred: the pool stays empty and the gradients are the immediate path's."""
    model = _model(gpu, "tiny")
    x, y = _batch(gpu)
    pool = ops.ColsumPool()
    assert _deferred.active() is None

    def run(scope):
        for p in model.parameters():
            p.grad = None
        loss = model(x, y)
        if scope:
            with ops.deferred_colsums(pool):
                assert _deferred.active() is pool
                loss.backward()
                assert pool.pending() == 0
        else:
            loss.backward()
        return {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    want, got = run(False), run(True)
    assert pool.nbytes() == 0 and _deferred.active() is None
    for n in want:
        if _exact(n):
            assert torch.equal(got[n], want[n]), n
