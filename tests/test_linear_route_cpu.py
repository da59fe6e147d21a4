"""Which GEMM back-end ops/linear.py picks (forward_route, dgrad_route, the fused MLP's routes) against a literal
table: the answers of the hand-written dispatch chains these functions replaced, recorded from a sweep of that code
on the built extension (which holds the kernels' shape rules, so the test needs the extension but no GPU: a
stand-in carries the three tensor properties the predicates read)."""
import importlib
import types

import pytest

torch = pytest.importorskip("torch")

from distributedvolunteercomputing_amd import config  # noqa: E402

L = importlib.import_module("distributedvolunteercomputing_amd.ops.linear")  # the module, not ops.linear()


@pytest.fixture(scope="module", autouse=True)
def C():
    from distributedvolunteercomputing_amd.ops._lib import native

    try:
        return native()
    except RuntimeError as e:  # the extension is built by __graft_entry__.build() / _build; CPU-only rules
        pytest.skip(str(e))


def _t(*shape, contiguous=True):
    """Stands in for a bf16 GPU tensor (a weight that requires grad, when given a shape)."""
    t = types.SimpleNamespace(is_cuda=True, dtype=torch.bfloat16, is_contiguous=lambda: contiguous, requires_grad=True)
    if shape:
        t.shape, t.dim = shape, lambda: len(shape)
        t.numel = lambda: int(torch.Size(shape).numel())
    return t


# y[M, N] = x[M, K] w[N, K]^T: M, N, K, config flip -> forward route without and with a bias, input-gradient route
# without and with a W^T handle
LINEAR = [
    # the default config at the GPT-2-small bench shapes: qkv, proj, fc, fc2, LM head
    (65536, 2304, 768, {}, "lib", "lib", "ps", "lib_nt"),
    (65536, 768, 768, {}, "lib", "lib", "ps", "lib_nt"),
    (65536, 3072, 768, {}, "lib", "lib", "lib_nn", "lib_nt"),
    (65536, 768, 3072, {}, "lib", "lib", "ps", "lib_nt"),
    (65536, 50304, 768, {}, "lib", "lib", "lib_nn", "lib_nt"),
    (65536, 2304, 768, {"dgrad_nt_attn": False}, "lib", "lib", "ps", "ps"),
    (65536, 768, 768, {"dgrad_ps": False}, "lib", "lib", "lib_nn", "lib_nt"),
    # gemm = "vcx": the LM head's forward stays on the library, its input gradient is gemm_nt's
    (65536, 50304, 768, {"gemm": "vcx"}, "lib", "lib", "nt", "nt"),
    (65536, 2304, 768, {"gemm": "vcx"}, "nt", "nt", "nt", "nt"),
    (65536, 768, 3072, {"gemm": "vcx"}, "nt", "nt", "nt", "nt"),
    (4096, 256, 256, {"gemm": "vcx"}, "nt", "nt", "nt", "nt"),
    (65536, 768, 768, {"gemm": "vcx", "gemm_fwd": "vcx"}, "nt", "nt", "nt", "nt"),
    (65536, 2304, 768, {"gemm_fwd": "vcx"}, "f", "f", "f", "f"),
    (65536, 50304, 768, {"gemm_fwd": "vcx"}, "f", "f", "f", "f"),
    (300, 128, 192, {"gemm_fwd": "vcx"}, "f", "f", "lib_nn", "lib_nt"),
    (300, 192, 128, {"gemm_fwd": "vcx"}, "lib", "lib", "f", "f"),
    # GPT-2 medium
    (65536, 4096, 1024, {}, "lib", "lib", "lib_nn", "lib_nt"),
    (65536, 1024, 1024, {}, "lib", "lib", "ps", "lib_nt"),
    (65536, 50304, 1024, {}, "lib", "lib", "lib_nn", "lib_nt"),
    (4096, 1024, 1024, {"dgrad_nt_attn": False}, "lib", "lib", "ps", "ps"),
    # ResNet-50 1x1 convolutions (no bias there; with one the vision GEMM is not taken)
    (401408, 64, 256, {"narrow_gemm": "vision"}, "narrow", "lib", "lib_nn", "lib_nt"),
    (401408, 256, 64, {"narrow_gemm": "vision"}, "lib", "lib", "narrow", "narrow"),
    (401408, 64, 64, {"narrow_gemm": "vision"}, "narrow", "lib", "narrow", "narrow"),
    (131072, 64, 32, {"narrow_gemm": "vision"}, "narrow", "lib", "narrow", "narrow"),
    (131072, 128, 512, {"narrow_gemm": "vision"}, "lib", "lib", "lib_nn", "lib_nt"),
    (401408, 128, 512, {"narrow_gemm": "vision"}, "narrow", "lib", "lib_nn", "lib_nt"),
    (65536, 64, 256, {"narrow_gemm": "vision"}, "lib", "lib", "lib_nn", "lib_nt"),
    (401408, 64, 256, {}, "lib", "lib", "lib_nn", "lib_nt"),
    # shapes no kernel takes, and the persistent GEMM's smallest
    (300, 96, 100, {}, "lib", "lib", "lib_nn", "lib_nt"),
    (300, 33, 17, {"gemm": "vcx", "gemm_fwd": "vcx", "narrow_gemm": "vision"}, "lib", "lib", "lib_nn", "lib_nt"),
    (300, 256, 256, {}, "lib", "lib", "lib_nn", "lib_nt"),
    (4096, 256, 256, {}, "lib", "lib", "ps", "lib_nt"),
]

# mlp_gelu(x[M, C], w1[F, C], b1, w2[C, F]): M, C, F, config flip -> mode, fc2 forward route, fc input-gradient route
# without and with a W1^T handle, mlp_wants_wt
MLP = [
    (65536, 768, 3072, {}, "ps", "lib", "lib_nn", "lib_nt", (True, True)),
    (65536, 768, 3072, {"fc_dgrad_nt": False}, "ps", "lib", "lib_nn", "lib_nn", (False, True)),
    (65536, 768, 3072, {"gemm_fwd": "vcx"}, "ps", "f", "lib_nn", "lib_nt", (True, True)),
    (65536, 768, 3072, {"gemm": "vcx"}, "ps", "lib", "lib_nn", "lib_nt", (True, True)),
    (65536, 768, 3072, {"mlp": "lib", "gemm": "vcx"}, "nt", "nt", "nt", "nt", (True, True)),
    (65536, 1024, 4096, {}, "ps", "lib", "lib_nn", "lib_nt", (True, True)),
    (4096, 256, 1024, {}, "ps", "lib", "lib_nn", "lib_nt", (True, True)),
    # unfused: two linear layers, each asked for itself
    (65536, 768, 3072, {"mlp": "lib"}, None, None, None, None, (False, True)),
    (65536, 768, 3072, {"mlp": "lib", "dgrad_ps": False}, None, None, None, None, (False, False)),
    (300, 256, 1024, {}, None, None, None, None, (False, False)),
    (4096, 100, 400, {}, None, None, None, None, (False, False)),
]


def test_table_covers_every_route():
    assert {r[4] for r in LINEAR} | {r[5] for r in LINEAR} == {"nt", "f", "narrow", "lib"}
    assert {r[6] for r in LINEAR} | {r[7] for r in LINEAR} == {"nt", "f", "narrow", "ps", "lib_nt", "lib_nn"}


@pytest.mark.parametrize("M,N,K,flip,fwd,fwd_bias,dgrad,dgrad_handle", LINEAR)
def test_linear_routes(M, N, K, flip, fwd, fwd_bias, dgrad, dgrad_handle):
    t = _t()
    with config.override(**flip):
        assert L.forward_route(M, N, K, t, None) == fwd
        assert L.forward_route(M, N, K, t, _t()) == fwd_bias
        assert L.dgrad_route(M, N, K, t, handle=False) == dgrad
        assert L.dgrad_route(M, N, K, t, handle=True) == dgrad_handle
        # the model makes W^T ahead of the backward exactly where the backward would make its own
        assert L.linear_wants_wt(M, _t(N, K), t) == (dgrad != "lib_nn")


def test_forward_bias_conditions():
    """gemm_f takes a bias only when it is contiguous; the vision GEMM takes none."""
    with config.override(gemm_fwd="vcx"):
        assert L.forward_route(300, 128, 192, _t(), _t(contiguous=False)) == "lib"
    with config.override(narrow_gemm="vision"):
        assert L.forward_route(131072, 64, 32, _t(), _t()) == "lib"


@pytest.mark.parametrize("M,C_,F_,flip,mode,fc2,dgrad,dgrad_handle,wants", MLP)
def test_mlp_routes(M, C_, F_, flip, mode, fc2, dgrad, dgrad_handle, wants):
    x, w1, w2 = _t(M, C_), _t(F_, C_), _t(C_, F_)
    with config.override(**flip):
        assert L._mlp_mode(x, w1, w2) == mode
        assert L.mlp_wants_wt(x, w1, w2) == wants
        if mode is None:
            assert wants == (L.dgrad_route(M, F_, C_, x, handle=False) != "lib_nn",
                             L.dgrad_route(M, C_, F_, x, handle=False) != "lib_nn")
            return
        assert L._mlp_routes(mode, M, C_, F_, x, handle=False) == (fc2, dgrad)
        assert L._mlp_routes(mode, M, C_, F_, x, handle=True) == (fc2, dgrad_handle)
        # fc: W1^T is worth making when the backward would read a handle; fc2's fused input gradient always reads W2^T
        assert wants == (dgrad_handle != "lib_nn", True)
