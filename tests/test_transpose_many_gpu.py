"""transpose_bf16_many (csrc/kernels/gemm.hip + job_table.h): many weight transposes in one launch, every output
bit-equal to ``w.t().contiguous()`` and to ``transpose_bf16``; job lists of 1, 4 and 49 matrices mixing the 16-B
body's shapes, ragged ones and the scalar body's, an empty list, a list past the per-launch cap, preset outputs."""
import pytest
import torch

from distributedvolunteercomputing_amd import ops

pytestmark = pytest.mark.gpu

# 768 x 768 .. 768 x 3072: GPT-2-small weights; 64 x 8, 1 x 136, 200 x 136: one tile / one row / ragged tiles on the
# 16-B body (200 x 136 has R, Cc % 8 == 0); 77 x 50, 65 x 129: the scalar body (a dimension that is no multiple of 8)
SHAPES = [(768, 768), (2304, 768), (768, 3072), (64, 8), (1, 136), (200, 136), (77, 50), (65, 129)]


def _mats(n, gpu, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(SHAPES[i % len(SHAPES)], generator=g).to(device=gpu, dtype=torch.bfloat16) for i in range(n)]


def _check(ws, outs):
    C = ops.native()
    assert len(outs) == len(ws)
    for w, o in zip(ws, outs):
        assert o.shape == (w.shape[1], w.shape[0]) and o.is_contiguous()
        assert torch.equal(o, w.t().contiguous())
        assert torch.equal(o, C.transpose_bf16(w))


@pytest.mark.parametrize("n", [1, 4, 49])
def test_transpose_many_matches_single(gpu, n):
    ws = _mats(n, gpu, seed=n)
    outs, launches = ops.native().transpose_bf16_many(ws)
    assert launches == 1
    _check(ws, outs)
    _check(ws, ops.transpose_weights(ws))


def test_transpose_many_unaligned_pointer_takes_scalar_body(gpu):
    """A 16 x 24 matrix whose storage starts 2 bytes into an allocation: shape fit for the 16-B body, pointer not."""
    base = torch.randn(16 * 24 + 1, device=gpu).to(torch.bfloat16)
    w = base[1:].view(16, 24)
    assert w.data_ptr() % 16 != 0 and w.is_contiguous()
    ws = [w, _mats(1, gpu)[0]]
    outs, _ = ops.native().transpose_bf16_many(ws)
    _check(ws, outs)


def test_transpose_many_empty_list_launches_nothing(gpu):
    outs, launches = ops.native().transpose_bf16_many([])
    assert outs == [] and launches == 0
    assert ops.transpose_weights([]) == []


def test_transpose_many_splits_past_the_cap(gpu):
    C = ops.native()
    cap = C.JOB_TABLE_CAP
    small = [s for s in SHAPES if s[0] * s[1] < 1 << 16]
    g = torch.Generator(device="cpu").manual_seed(7)
    for n, want in ((cap, 1), (cap + 1, 2), (2 * cap + 3, 3)):
        ws = [torch.randn(small[i % len(small)], generator=g).to(device=gpu, dtype=torch.bfloat16) for i in range(n)]
        outs, launches = C.transpose_bf16_many(ws)
        assert launches == want
        for w, o in zip(ws, outs):
            assert torch.equal(o, w.t().contiguous())


def test_transpose_many_writes_preset_outputs_in_place(gpu):
    """The persistent-buffer form: a second call with the first call's outputs rewrites them in place with the
    weights' new values; outputs of the wrong shapes are replaced, not written."""
    ws = _mats(9, gpu, seed=3)
    outs = ops.transpose_weights(ws)
    ptrs = [o.data_ptr() for o in outs]
    for w in ws:
        w.mul_(-2.0)
    again = ops.transpose_weights(ws, outs)
    assert [o.data_ptr() for o in again] == ptrs
    _check(ws, again)
    other = ops.transpose_weights(ws[:3], outs)  # not the list of these weights: fresh outputs
    assert all(o.data_ptr() not in ptrs for o in other)
    _check(ws[:3], other)
    with pytest.raises(RuntimeError):
        ops.native().transpose_bf16_many(ws[:2], [outs[1], outs[0]])
