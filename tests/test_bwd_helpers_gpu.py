"""Weight transposes made once per forward (config.bwd_batch: GPT2._weight_transposes -> transpose_bf16_many) and
the fused MLP's fc input gradient as an NT GEMM on fc_w^T (config.fc_dgrad_nt), on a 2-layer GPT-2 of width 256
(the smallest the persistent GEMM takes: K >= 256, 256-row tiles), T = 128, vocabulary 512, with flat gradient
buffers as LocalSGDTrainer sets them up.

The batched transposes move bits, so with the NT input gradients (fc_dgrad_nt, lmhead_dgrad_nt) off the gradients
must be the immediate path's bit for bit.
Two gradients of this model are summed with floating-point atomics whatever the switches say -- every fc bias
(gemm_ps.hip's epilogue adds per-wave column sums into one fp32 row) and the token embedding (embed.hip adds the
rows of repeated tokens) -- so two runs of ONE path already differ there in the order of an fp32 sum of <= 256
terms, which the rounding to bf16 turns into at most one bf16 ulp on an element. Those are held element by
element to one bf16 ulp of the larger value (2^-7 relative at most), plus 2^-16 of the tensor's largest magnitude
for an element whose terms cancel (the fp32 rounding of a sum of n <= 256 terms is at most n 2^-24 = 2^-16 of the
partial sums, which are of the order of the tensor's values); every other gradient and the loss to torch.equal."""
import importlib

import pytest
import torch

from distributedvolunteercomputing_amd import config, ops
from distributedvolunteercomputing_amd.models.gpt2 import GPT2, GPT2Config
from distributedvolunteercomputing_amd.parallel.flat_params import FlatParams

pytestmark = pytest.mark.gpu

L = importlib.import_module("distributedvolunteercomputing_amd.ops.linear")  # the module, not ops.linear()

OFF = dict(bwd_batch=False, fc_dgrad_nt=False, lmhead_dgrad_nt=False)
ON = dict(bwd_batch=True, fc_dgrad_nt=False, lmhead_dgrad_nt=False)  # the transposes alone: bit-identical by construction
B, T = 2, 128


def _cfg():
    return GPT2Config(vocab_size=512, padded_vocab=512, n_ctx=T, n_layer=2, n_head=4, n_embd=256)


def _model(gpu, flat=True, seed=11):
    model = GPT2(_cfg())
    model.reset_parameters(seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1:  # biases and gains away from their 0 / 1 initial values
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    model = model.to(device=gpu, dtype=torch.bfloat16)
    return model, (FlatParams(model, device=gpu) if flat else None)


def _batch(gpu, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randint(0, 512, (B, T + 1), generator=g).to(gpu)
    return t[:, :-1].contiguous(), t[:, 1:].contiguous()


def _zero(model, flat):
    if flat is not None:
        flat.zero_grad()
    else:
        for p in model.parameters():
            p.grad = None


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _fwd_bwd(model, flat, x, y, switches):
    with config.override(**switches):
        _zero(model, flat)
        loss = model(x, y)
        loss.backward()
    return loss.detach().clone(), _grads(model)


def _atomic(name):
    return name == "wte" or name.endswith(".fc_b")


def _assert_same(got, want, tied_l2=False):
    """tied_l2: the tied embedding's two contributions were rounded to bf16 separately on one side (autograd's
    accumulation) and together on the other (the flat buffer), which no per-element bound in ulps of the sum
    covers where they cancel: wte is then held to 2^-7 relative L2 (one ulp on every element at the worst)."""
    (gl, gg), (wl, wg) = got, want
    assert torch.equal(gl, wl), (float(gl), float(wl))
    assert gg.keys() == wg.keys()
    for n in wg:
        a, b = gg[n].float(), wg[n].float()
        if n == "wte" and tied_l2:
            rel = float((a - b).norm() / b.norm())
            assert rel <= 2.0 ** -7, (n, rel)
        elif _atomic(n):
            bound = 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 2.0 ** -16 * float(b.abs().max())
            over = (a - b).abs() - bound
            assert float(over.max()) <= 0, (n, float(over.max()), int((over > 0).sum()))
        else:
            assert torch.equal(gg[n], wg[n]), (n, float((gg[n].float() - wg[n].float()).abs().max()))


@pytest.fixture()
def transposes(monkeypatch):
    """Counts the one-at-a-time transposes (ops.linear.transpose_weight) a block of code makes."""
    calls = []
    real = L.transpose_weight
    monkeypatch.setattr(L, "transpose_weight", lambda w: (calls.append(tuple(w.shape)), real(w))[1])
    return calls


def test_config_takes_the_paths_under_test(gpu):
    """At this size the MLP is on gemm_ps and the qkv / projection input gradients read W^T."""
    model, _ = _model(gpu)
    b0 = model.blocks[0]
    h = torch.empty(B, T, 256, device=gpu, dtype=torch.bfloat16)
    assert L._mlp_mode(h, b0.fc_w, b0.fc2_w) == "ps"
    assert L.linear_wants_wt(B * T, b0.attn_w, h) and L.linear_wants_wt(B * T, b0.proj_w, h)
    with config.override(fc_dgrad_nt=False):
        assert L.mlp_wants_wt(h, b0.fc_w, b0.fc2_w) == (False, True)
    with config.override(fc_dgrad_nt=True):
        assert L.mlp_wants_wt(h, b0.fc_w, b0.fc2_w) == (True, True)


def test_bitwise_match_and_no_transposes_left_in_the_backward(gpu, transposes):
    model, flat = _model(gpu)
    x, y = _batch(gpu)
    want = _fwd_bwd(model, flat, x, y, OFF)
    # in the backward: attn_w, proj_w, fc2_w of two blocks, and the LM head's wte (a vocabulary this small is on gemm_ps)
    assert len(transposes) == 7 and model._wt_bufs is None
    del transposes[:]
    got = _fwd_bwd(model, flat, x, y, ON)
    assert transposes == [] and len(model._wt_bufs) == 7
    _assert_same(got, want)
    ws = [w for blk in model.blocks for w in (blk.attn_w, blk.proj_w, blk.fc2_w)] + [model.wte]
    for w, wt in zip(ws, model._wt_bufs):
        assert torch.equal(wt, w.t().contiguous())


def test_weights_rewritten_in_place_between_steps(gpu):
    """Staleness: every weight overwritten through the flat buffer (as the flat AdamW kernel does it: no version
    bump on the parameters) between two forward/backward passes; the second pass is the immediate path's on the new
    weights, and the persistent W^T buffers were reused, not reallocated."""
    model, flat = _model(gpu)
    x, y = _batch(gpu)
    _fwd_bwd(model, flat, x, y, ON)
    ptrs = [t.data_ptr() for t in model._wt_bufs]
    versions = [p._version for p in model.parameters()]
    other, _ = _model(gpu, seed=23)
    with torch.no_grad():
        flat.param.copy_(_flat_of(other, flat))
    assert [p._version for p in model.parameters()] == versions
    got = _fwd_bwd(model, flat, x, y, ON)
    assert [t.data_ptr() for t in model._wt_bufs] == ptrs
    want = _fwd_bwd(model, flat, x, y, OFF)
    _assert_same(got, want)


def _flat_of(other, flat):
    """The parameters of `other` (same architecture) laid out as `flat`'s parameter buffer."""
    out = torch.zeros_like(flat.param)
    byname = dict(other.named_parameters())
    for s in flat.segments:
        out[s.offset:s.offset + s.numel] = byname[s.name].detach().reshape(-1)
    return out


def test_two_backward_passes_on_one_graph(gpu, transposes):
    """One forward, then backward(retain_graph=True) and backward again: the second pass still has its handles and
    accumulates onto the first exactly as the immediate path does. On a projection + fused MLP chain with the
    model's weights and flat gradient buffers, not the whole model: its embedding and loss ops release their
    state in their first backward pass (ops/embedding.py, ops/loss.py), with or without this change."""
    model, flat = _model(gpu)
    b0 = model.blocks[0]
    g = torch.Generator(device="cpu").manual_seed(9)
    h = torch.randn(B * T, 256, generator=g).to(device=gpu, dtype=torch.bfloat16)
    dy = torch.randn(B * T, 256, generator=g).to(device=gpu, dtype=torch.bfloat16)
    names = {"blocks.0.proj_w": b0.proj_w, "blocks.0.fc_w": b0.fc_w, "blocks.0.fc_b": b0.fc_b, "blocks.0.fc2_w": b0.fc2_w}

    def run(on, passes):
        flat.zero_grad()
        hi = h.clone().requires_grad_()
        with config.override(**(ON if on else OFF)):
            wts = ops.transpose_weights([b0.proj_w, b0.fc_w, b0.fc2_w]) if on else (None, None, None)
            y = ops.mlp_gelu(ops.linear(hi, b0.proj_w, wt=wts[0]), b0.fc_w, b0.fc_b, b0.fc2_w, w1t=wts[1], w2t=wts[2])
            loss = (y.float() * dy.float()).sum()
            for i in range(passes):
                loss.backward(retain_graph=i + 1 < passes)
        return loss.detach().clone(), {"h": hi.grad.clone(), **{n: p.grad.detach().clone() for n, p in names.items()}}

    want = run(False, 2)
    assert len(transposes) == 4  # proj_w and fc2_w, once per pass
    del transposes[:]
    got = run(True, 2)
    assert transposes == []
    _assert_same(got, want)
    once = run(True, 1)
    assert not torch.equal(once[1]["blocks.0.proj_w"], got[1]["blocks.0.proj_w"])  # the second pass did accumulate


def test_frozen_layernorm_parameters(gpu, transposes):
    """One LayerNorm's weight and bias frozen (requires_grad=False, so they are in no flat buffer and get no
    gradient): the handles still reach every op, and every other gradient is the immediate path's bit for bit."""
    model = GPT2(_cfg())
    model.reset_parameters(11)
    model = model.to(device=gpu, dtype=torch.bfloat16)
    frozen = (model.blocks[1].ln1_w, model.blocks[1].ln1_b)
    for p in frozen:
        p.requires_grad_(False)
    flat = FlatParams(model, device=gpu)
    assert len(flat.segments) == len(list(model.parameters())) - 2
    x, y = _batch(gpu)

    def run(switches):
        with config.override(**switches):
            flat.zero_grad()
            loss = model(x, y)
            loss.backward()
        return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}

    want = run(OFF)
    del transposes[:]
    got = run(ON)
    assert transposes == [] and len(model._wt_bufs) == 7
    assert all(p.grad is None for p in frozen)
    assert "blocks.1.ln1_w" not in got[1] and "blocks.0.ln1_w" in got[1]
    _assert_same(got, want)


def test_linear_with_a_handle_takes_the_nt_gemm(gpu, monkeypatch):
    """A linear layer given W^T at a shape no hand-written input-gradient kernel takes (3072 input-gradient columns
    of reduction: dgrad_ps_ok refuses K > 2304) computes dX = dY (W^T)^T on the NT library GEMM -- the LM head's
    path (config.lmhead_dgrad_nt). Against mm(dy, w): the same fp32 dot products summed in another order and
    rounded to bf16 once, so at most one bf16 ulp apart on an element (2^-7 relative L2 at the worst); the weight
    gradient does not depend on the handle."""
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(512, 768, generator=g).to(device=gpu, dtype=torch.bfloat16)
    w = (torch.randn(3072, 768, generator=g) * 0.02).to(device=gpu, dtype=torch.bfloat16).requires_grad_()
    dy = torch.randn(512, 3072, generator=g).to(device=gpu, dtype=torch.bfloat16)
    assert not L.linear_wants_wt(512, w, x)
    seen = []
    real = L.mm
    monkeypatch.setattr(L, "mm", lambda a, b, trans_a=False, trans_b=False, bias=None: (
        seen.append((tuple(a.shape), tuple(b.shape), trans_b)), real(a, b, trans_a, trans_b, bias))[1])
    outs = {}
    for handle in (False, True):
        xi = x.clone().requires_grad_()
        w.grad = None
        wt = ops.transpose_weights([w.detach()])[0] if handle else None
        yo = ops.linear(xi, w, wt=wt)
        del seen[:]
        yo.backward(dy)
        assert seen == [((512, 3072), (768, 3072), True) if handle else ((512, 3072), (3072, 768), False)]
        outs[handle] = (yo.detach().clone(), xi.grad.clone(), w.grad.clone())
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][2], outs[False][2])
    ref = real(dy, w.detach()).float()
    assert torch.equal(outs[False][1].float(), ref)
    assert float((outs[True][1].float() - ref).norm() / ref.norm()) <= 2.0 ** -7


# y[M, N] = x[M, K] w[N, K]^T at the smallest shape each back-end's *_supported takes (asked of the extension on the
# CPU): gemm_nt 256 x 256 x 128, gemm_f 300 x 128 x 192, gemm_ps 256^3, the vision GEMM from 131072 rows with <= 64
# columns and K % 32 == 0; 96 x 100 x 100 is no kernel's. An input gradient is the GEMM [M, K] = [M, N] [K, N]^T, so
# its shapes have N and K swapped.
_VCX, _F, _NARROW = dict(gemm="vcx"), dict(gemm_fwd="vcx"), dict(narrow_gemm="vision")
DISPATCH = [  # direction, route, config flip, M, N, K, bias, handle
    ("fwd", "nt", _VCX, 256, 256, 128, True, False),
    ("fwd", "f", _F, 300, 128, 192, True, False),
    ("fwd", "narrow", _NARROW, 131072, 64, 32, False, False),
    ("fwd", "lib", {}, 96, 100, 100, True, False),
    ("dgrad", "nt", _VCX, 256, 128, 256, False, False),
    ("dgrad", "nt", _VCX, 256, 128, 256, False, True),
    ("dgrad", "f", _F, 300, 192, 128, False, False),
    ("dgrad", "f", _F, 300, 192, 128, False, True),
    ("dgrad", "narrow", _NARROW, 131072, 32, 64, False, False),
    ("dgrad", "narrow", _NARROW, 131072, 32, 64, False, True),
    ("dgrad", "ps", {}, 256, 256, 256, True, False),
    ("dgrad", "ps", dict(dgrad_nt_attn=False), 256, 256, 256, False, True),
    ("dgrad", "lib_nt", {}, 256, 256, 256, False, True),  # a handle moves the gemm_ps shape to the NT library GEMM
    ("dgrad", "lib_nt", {}, 96, 100, 100, False, True),
    ("dgrad", "lib_nn", {}, 96, 100, 100, True, False),
]


@pytest.mark.parametrize("direction,route,flip,M,N,K,bias,handle", DISPATCH)
def test_dispatch_runs_what_the_route_names(gpu, monkeypatch, transposes, direction, route, flip, M, N, K, bias, handle):
    """One forward and backward of ops.linear with every GEMM entry point spied on: the one that ran is the one
    forward_route / dgrad_route named (which is the one the config flip was meant to select), and the backward made
    a transpose of its own exactly when it had no handle and its route reads W^T. The result is held to the fp32
    product rounded to bf16 once: 2^-7 relative L2 at the worst (one bf16 ulp on every element)."""
    ran = []

    def spy(obj, name, label):
        real = getattr(obj, name)

        def wrapper(*a, **kw):
            ran.append(label(*a, **kw) if callable(label) else label)
            return real(*a, **kw)

        monkeypatch.setattr(obj, name, wrapper)

    spy(L, "gemm_nt", "nt")
    spy(L, "gemm_f", "f")
    spy(L, "narrow_gemm", "narrow")
    spy(ops.native(), "gemm_ps", "ps")
    spy(L, "mm", lambda a, b, trans_a=False, trans_b=False, bias=None: "lib_nt" if trans_b else "lib_nn")
    g = torch.Generator(device="cpu").manual_seed(17)
    x = torch.randn(M, K, generator=g).to(device=gpu, dtype=torch.bfloat16).requires_grad_()
    w = (torch.randn(N, K, generator=g) * 0.05).to(device=gpu, dtype=torch.bfloat16).requires_grad_()
    b = (torch.randn(N, generator=g) * 0.05).to(device=gpu, dtype=torch.bfloat16).requires_grad_() if bias else None
    dy = torch.randn(M, N, generator=g).to(device=gpu, dtype=torch.bfloat16)
    with config.override(**flip):
        wt = ops.transpose_weights([w.detach()])[0] if handle else None
        want_fwd, want_dgrad = L.forward_route(M, N, K, x, b), L.dgrad_route(M, N, K, dy, handle)
        assert (want_fwd if direction == "fwd" else want_dgrad) == route
        y = ops.linear(x, w, b, wt=wt)
        assert ran == ["lib_nt" if want_fwd == "lib" else want_fwd] and transposes == []  # x W^T on the library is an NT GEMM
        del ran[:]
        y.backward(dy)
        assert ran == [want_dgrad]
        assert len(transposes) == (1 if not handle and want_dgrad != "lib_nn" else 0)
    ref_y = x.detach().float() @ w.detach().float().t() + (b.detach().float() if bias else 0)
    ref_dx = dy.float() @ w.detach().float()
    assert float((y.detach().float() - ref_y).norm() / ref_y.norm()) <= 2.0 ** -7
    assert float((x.grad.float() - ref_dx).norm() / ref_dx.norm()) <= 2.0 ** -7


def test_without_preset_flat_buffers(gpu, transposes):
    """No preset .grad buffers: the gradients come back through autograd, the same with the switch on and off, and
    equal to the flat-buffer run's (one contribution per parameter, rounded to bf16 once on either route; the tied
    embedding gets two: _assert_same, tied_l2)."""
    model, _ = _model(gpu, flat=False)
    x, y = _batch(gpu)
    want = _fwd_bwd(model, None, x, y, OFF)
    del transposes[:]
    got = _fwd_bwd(model, None, x, y, ON)
    assert transposes == []
    _assert_same(got, want)
    fmodel, flat = _model(gpu)
    _assert_same(got, _fwd_bwd(fmodel, flat, x, y, ON), tied_l2=True)


def test_graph_capture_replays_follow_the_weights(gpu):
    """The step captured as one linear stream (torch.cuda.graph), replayed twice with a weight update in between:
    the transposes are part of the graph, so each replay's gradients are the eager immediate path's on the weights
    of that moment."""
    model, flat = _model(gpu)
    x, y = _batch(gpu)
    other = _flat_of(_model(gpu, seed=29)[0], flat)
    first = flat.param.clone()
    with config.override(**ON):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                flat.zero_grad()
                model(x, y).backward()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            flat.zero_grad()
            loss = model(x, y)
            loss.backward()
    for weights in (first, other):
        with torch.no_grad():
            flat.param.copy_(weights)
        graph.replay()
        torch.cuda.synchronize()
        got = (loss.detach().clone(), _grads(model))
        _assert_same(got, _fwd_bwd(model, flat, x, y, OFF))
    del graph


def test_fc_input_gradient_nt_matches_unfused(gpu, monkeypatch):
    """config.fc_dgrad_nt: the input gradient of mlp_gelu through the NT GEMM on W1^T against the library +
    bias_gelu path, at the tolerance test_kernels_train_gpu.py::test_mlp_gelu_persistent_matches_unfused holds the
    same quantity to; the NT form is what ran."""
    torch.manual_seed(1)

    def bf(t):
        return t.to(torch.bfloat16)

    x = bf(torch.randn(1024, 768, device=gpu))
    w1 = bf(torch.randn(3072, 768, device=gpu) * 0.02).requires_grad_()
    b1 = bf(torch.randn(3072, device=gpu) * 0.02).requires_grad_()
    w2 = bf(torch.randn(768, 3072, device=gpu) * 0.02).requires_grad_()
    dy = bf(torch.randn(1024, 768, device=gpu))
    seen = []
    real = L.mm
    monkeypatch.setattr(L, "mm", lambda a, b, trans_a=False, trans_b=False, bias=None: (
        seen.append((tuple(a.shape), tuple(b.shape), trans_b)), real(a, b, trans_a, trans_b, bias))[1])
    outs = {}
    for mode in ("lib", "nt", "nn"):
        with config.override(mlp="lib" if mode == "lib" else "fused", fc_dgrad_nt=mode == "nt"):
            xi = x.clone().requires_grad_()
            for p in (w1, b1, w2):
                p.grad = None
            # the reference gets no handles: a linear layer that is given one uses it
            w1t, w2t = (None, None) if mode == "lib" else ops.transpose_weights([w1.detach(), w2.detach()])
            yo = ops.mlp_gelu(xi, w1, b1, w2, w1t=w1t, w2t=w2t)
            del seen[:]  # the forward's fc2 GEMM has the same shapes
            yo.backward(dy)
            assert (((1024, 3072), (768, 3072), True) in seen) == (mode == "nt"), seen
            outs[mode] = [t.float().clone() for t in (xi.grad, w1.grad, b1.grad, w2.grad)]
    for a, b in zip(outs["lib"], outs["nt"]):
        assert (a - b).norm() / b.norm() < 2e-2
    # against the NN form of the same GEMM: two bf16 roundings of one fp32 dot product summed in two orders
    assert (outs["nt"][0] - outs["nn"][0]).norm() / outs["nn"][0].norm() < 2.0 ** -7
