"""The attention backward's workgroup shape (mfma_attention.hip, BW_THREADS): at d_head 64 both
backward kernels run 4-wave workgroups of 128 rows (keys), two per CU, with the blocks of every
slice dispatched heaviest first.  What that mapping stresses, against the oracle chain: a ragged
last block, more backward blocks per slice than the forward left clamp-bound slots, one slice, slice
counts that do not divide by the XCD count, both layouts of y / grad_y, and bf16 storage."""
import pytest
import torch

from test_gpu_fused_attention import CLAMP, causal_indices, oracle_chain
from test_gpu_mfma_attention import BF16_ULP, _scores_on_the_clamp

pytestmark = pytest.mark.gpu

SHAPES = [                             # (N, H, S, Z, d_head)
    (1, 1, 320, 32, 64),               # one slice; 320 = 2.5 blocks of 128 rows: ragged last block
    (2, 3, 640, 64, 64),               # 5 blocks per slice, 6 slices (not a multiple of 8 XCDs)
    (1, 2, 2048, 128, 64),             # 16 backward blocks per slice against 8 forward bound slots
    (1, 1, 128, 16, 64),               # one block
    (3, 1, 96, 8, 64),                 # S below one block
    (1, 3, 320, 32, 128),              # d_head 128 (the 8-wave shape) at a ragged S
]


def _want(q, k, v, gy, indices, scale):
    """grad_q, grad_k, grad_v of the oracle chain (as test_gpu_mfma_attention does)."""
    import numpy as np
    from oracle import ext_stub
    N, S, H, E = q.shape
    B, Z = N * H, indices.size(-1) // S
    scores, attn, _ = oracle_chain(indices, q, k, v, scale)
    flat = lambda t: t.transpose(1, 2).contiguous().view(B, S, E)       # noqa: E731
    heads = lambda t: t.view(N, H, S, E).transpose(1, 2)                  # noqa: E731
    indptr = torch.arange(0, S * Z + 1, Z, dtype=torch.int32)
    f, t = torch.scalar_tensor(False), torch.scalar_tensor(True)
    raw_scores = ext_stub.sddmm_forward_cuda(f, t, indptr, indices, flat(q), flat(k)) * np.float32(scale)
    dp = ext_stub.sddmm_forward_cuda(f, t, indptr, indices, gy, flat(v))
    ds = ext_stub.softmax_backward_cuda(indptr, indices, attn, dp)
    raw = torch.where(raw_scores.abs() < CLAMP, ds * np.float32(scale), torch.zeros_like(ds))
    return (heads(ext_stub.spmm_forward_cuda(f, f, indptr, indices, raw, flat(k))),
            heads(ext_stub.spmm_forward_cuda(t, f, indptr, indices, raw, flat(q))),
            heads(ext_stub.spmm_forward_cuda(t, f, indptr, indices, attn, gy)))


def _run(q, k, v, gy, indices, scale, gt):
    from naive_gpt import ext
    S = q.size(1)
    tiles = ext.attention_mfma_prepare(indices.cuda(), S)
    y, row_sum = ext.attention_mfma_forward(tiles, q.cuda(), k.cuda(), v.cuda(), scale, CLAMP,
                                            y_transposed=gt)
    gy_in = (gy.transpose(1, 2).contiguous() if gt else gy).to(device='cuda', dtype=q.dtype)
    return [ext.attention_mfma_backward(tiles, q.cuda(), k.cuda(), v.cuda(), y, gy_in, row_sum,
                                        scale, CLAMP, transposed=gt) for _ in range(2)]


@pytest.mark.parametrize('gt', [False, True])
@pytest.mark.parametrize('N,H,S,Z,E', SHAPES)
def test_backward_blocks_match_oracle_chain(N, H, S, Z, E, gt):
    gen = torch.Generator().manual_seed(3 * N + S + Z + E)
    q, k, v = [torch.randn([N, S, H, E], generator=gen) for _ in range(3)]
    q = q * 3.0                                    # some scores beyond the clamp
    gy = torch.randn([N * H, S, E], generator=gen)
    indices = causal_indices(N * H, S, Z, gen)
    scale = E ** -0.5
    wants = _want(q, k, v, gy, indices, scale)
    first, again = _run(q, k, v, gy, indices, scale, gt)
    for got, rep, want, name in zip(first, again, wants, ('grad_q', 'grad_k', 'grad_v')):
        assert torch.equal(got, rep), name        # no order of work depends on the dispatch
        got = got.cpu()
        assert torch.isfinite(got).all(), name
        err = (got - want).abs().max().item()
        assert torch.allclose(got, want, rtol=1e-3, atol=2e-4 * want.abs().max().item()), \
            (name, err, want.abs().max().item())


@pytest.mark.parametrize('gt', [False, True])
@pytest.mark.parametrize('N,H,S,Z,E', [(1, 1, 320, 32, 64), (1, 2, 640, 64, 64), (2, 3, 96, 8, 128)])
def test_backward_blocks_bf16_storage(N, H, S, Z, E, gt):
    """bf16 storage takes the same shape: against the oracle on the bf16-rounded inputs, with
    test_gpu_mfma_attention's bar for bf16 storage (the stored y feeds delta: one more rounding)."""
    gen = torch.Generator().manual_seed(5 * N + S + E)
    q, k, v = [torch.randn([N, S, H, E], generator=gen).bfloat16() for _ in range(3)]
    gy = torch.randn([N * H, S, E], generator=gen).bfloat16()
    indices = causal_indices(N * H, S, Z, gen)
    scale = E ** -0.5
    wants = _want(q.float(), k.float(), v.float(), gy.float(), indices, scale)
    first, again = _run(q, k, v, gy, indices, scale, gt)
    for got, rep, want, name in zip(first, again, wants, ('grad_q', 'grad_k', 'grad_v')):
        assert got.dtype == torch.bfloat16 and torch.equal(got, rep), name
        got = got.float().cpu()
        bar = 4e-3 * want.abs().max() + BF16_ULP * want.abs()
        assert ((got - want).abs() <= bar).all(), (name, (got - want).abs().max().item())


@pytest.mark.parametrize('gt', [False, True])
@pytest.mark.parametrize('N,H,S,Z,E', [(1, 1, 2048, 128, 64), (1, 2, 640, 64, 64)])
def test_clamp_guard_reads_the_forward_slots(N, H, S, Z, E, gt):
    """The exact clamp mask needs the norm bounds of every FORWARD block of the slice (256 rows
    each).  At S = 2048 the backward has 16 blocks per slice and the forward 8 bound slots; at
    S = 640 it has 5 against 3.  Scores sit within 2^-15 of the clamp: a guard that read the wrong
    slots would be off (or read past the slice's slots) and flip cells."""
    import numpy as np
    from oracle import ext_stub
    B = N * H
    q, k, v, indices, scale = _scores_on_the_clamp(N, H, S, Z, E, 13 * S + E, 2.0 ** -15)
    gen = torch.Generator().manual_seed(9)
    gy = torch.randn([B, S, E], generator=gen)
    flat = lambda t: t.transpose(1, 2).contiguous().view(B, S, E)       # noqa: E731
    indptr = torch.arange(0, S * Z + 1, Z, dtype=torch.int32)
    f, t = torch.scalar_tensor(False), torch.scalar_tensor(True)
    raw_scores = ext_stub.sddmm_forward_cuda(f, t, indptr, indices, flat(q), flat(k)) * np.float32(scale)
    near = ((raw_scores.abs() - CLAMP).abs() < CLAMP * 2.0 ** -14)
    assert near.sum() > 0.3 * B * S, 'the construction put too few scores on the clamp'
    want_q, want_k, _ = _want(q, k, v, gy, indices, scale)
    (gq, gk, _), _ = _run(q, k, v, gy, indices, scale, gt)
    for got, want, name in ((gq, want_q, 'grad_q'), (gk, want_k, 'grad_k')):
        rel = ((got.cpu() - want).abs().max() / want.abs().max()).item()
        assert rel < 2e-4, (name, rel)
