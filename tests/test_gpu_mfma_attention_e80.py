"""d_head 80 (OPT-2.7B: d_model 2560, 32 heads) on the matrix-core attention kernels and the fused
PQ loss at M = 10 subspaces: kernels against the oracle chain, the layers against the
separate-operators path, and the contract / poisoned-buffer checks of the d_head 64 / 128 builds
reused at 80 through their modules' helpers."""
import pytest
import torch

import test_gpu_arith_contract as C
import test_gpu_fused_attention as F
import test_gpu_mfma_attention as MA
import test_gpu_poisoned_buffers as P

pytestmark = pytest.mark.gpu
E = 80
CLAMP = 10.0
SHAPES = [(2, 16, 512, 64), (2, 16, 80, 8), (1, 2, 2048, 256)]     # (N, H, S, Z)


def _inputs(N, H, S, Z, seed, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    q, k, v = [torch.randn([N, S, H, E], generator=gen) for _ in range(3)]
    gy = torch.randn([N * H, S, E], generator=gen)
    if dtype == torch.bfloat16:
        q, k, v, gy = (t.bfloat16().float() for t in (q, k, v, gy))
    idx = F.causal_indices(N * H, S, Z, gen)
    return q, k, v, gy, idx


def _run(idx, q, k, v, gy, gt, dtype=torch.float32, compact=False):
    from naive_gpt import ext
    S = q.size(1)
    scale = E ** -0.5
    tiles = ext.attention_mfma_prepare(idx.cuda(), S, lookup_pattern=compact)
    qd, kd, vd = (t.to(dtype).cuda() for t in (q, k, v))
    y, row_sum = ext.attention_mfma_forward(tiles, qd, kd, vd, scale, CLAMP, y_transposed=gt)
    gyd = (gy.transpose(1, 2).contiguous() if gt else gy).to(dtype).cuda()
    gq, gk, gv = ext.attention_mfma_backward(tiles, qd, kd, vd, y, gyd, row_sum, scale, CLAMP, transposed=gt)
    if gt:
        y = y.transpose(1, 2)
    return [t.float().cpu() for t in (y, gq, gk, gv)]


def _close(got, want, name, rtol):
    err = (got.double() - want.double()).abs()
    bound = rtol * want.double().abs() + rtol * float(want.abs().max())
    assert (err <= bound).all(), '{}: worst |err| {:.3e} (max |want| {:.3e})'.format(
        name, float(err.max()), float(want.abs().max()))


@pytest.mark.parametrize('gt', [False, True])
@pytest.mark.parametrize('N,H,S,Z', SHAPES)
def test_e80_forward_and_gradients_match_the_oracle_chain(N, H, S, Z, gt):
    q, k, v, gy, idx = _inputs(N, H, S, Z, seed=S + Z)
    _, _, y_want = F.oracle_chain(idx, q, k, v, E ** -0.5)
    refs = P._attn_refs(idx, q, k, v, gy, E ** -0.5)
    y, gq, gk, gv = _run(idx, q, k, v, gy, gt)
    _close(y, y_want, 'y', 1e-3)
    for got, want, name in ((gq, refs[3], 'grad_q'), (gk, refs[4], 'grad_k'), (gv, refs[5], 'grad_v')):
        _close(got, want, name, 1e-3)


@pytest.mark.parametrize('gt', [False, True])
@pytest.mark.parametrize('N,H,S,Z', [(2, 16, 512, 64), (2, 16, 80, 8)])
def test_e80_bf16_storage_matches_the_oracle_on_rounded_inputs(N, H, S, Z, gt):
    q, k, v, gy, idx = _inputs(N, H, S, Z, seed=3 * S + Z, dtype=torch.bfloat16)
    refs = P._attn_refs(idx, q, k, v, gy, E ** -0.5)
    y, gq, gk, gv = _run(idx, q, k, v, gy, gt, dtype=torch.bfloat16)
    _close(y, refs[2], 'y', 1e-2)
    for got, want, name in ((gq, refs[3], 'grad_q'), (gk, refs[4], 'grad_k'), (gv, refs[5], 'grad_v')):
        _close(got, want, name, 1e-2)


@pytest.mark.parametrize('N,H,S,Z', SHAPES)
def test_e80_compact_tiles_equal_full_tiles_bit_for_bit(N, H, S, Z):
    q, k, v, gy, _ = _inputs(N, H, S, Z, seed=7 * S)
    gen = torch.Generator().manual_seed(S)
    idx = P._dead_key_indices(N * H, S, Z, gen, distinct=True)
    full = _run(idx, q, k, v, gy, False)
    compact = _run(idx, q, k, v, gy, False, compact=True)
    for a, b, name in zip(full, compact, ('y', 'grad_q', 'grad_k', 'grad_v')):
        assert torch.equal(a, b), name


def test_e80_forward_and_grad_q_are_deterministic():
    q, k, v, gy, idx = _inputs(2, 16, 512, 64, seed=11)
    first, second = _run(idx, q, k, v, gy, False), _run(idx, q, k, v, gy, False)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


@pytest.mark.parametrize('gt', [False, True])
@pytest.mark.parametrize('N,H,S,Z', [(2, 16, 512, 64), (1, 8, 80, 8), (1, 2, 2048, 256)])
def test_e80_clamp_mask_is_that_of_the_exact_scores(N, H, S, Z, gt):
    MA.test_clamp_mask_is_that_of_the_exact_scores(N, H, S, Z, E, gt)


@pytest.mark.parametrize('bf16', [False, True])
def test_e80_within_the_chain_bound(bf16):
    C.test_attention_mfma_within_the_chain_bound(1, 4, 256, 32, E, bf16)


# the registry's attention cases at d_head 80; test_gpu_guard_bands runs them between guard bands too
E80_CASES = [
    ('attention_mfma_prepare', P.Case('s320_e80_compact', P._mfma(1, 2, 320, 32, E, False, 'bits'), P.ATOMIC)),
    ('attention_mfma_forward', P.Case('s640_e80_yt', P._mfma(1, 2, 640, 64, E, True), P.ATOMIC)),
    ('attention_mfma_forward', P.Case('s2048_z256_e80', P._mfma(1, 1, 2048, 256, E, False), P.ATOMIC)),
    ('attention_mfma_backward', P.Case('s320_e80', P._mfma(1, 2, 320, 32, E, False), P.ATOMIC)),
    ('attention_mfma_backward', P.Case('s320_e80_gt', P._mfma(1, 2, 320, 32, E, True), P.ATOMIC)),
    ('attention_mfma_backward', P.Case('s320_e80_bf16', P._mfma(1, 2, 320, 32, E, False, bf16=True), P.ATOMIC)),
    ('attention_mfma_backward', P.Case('s320_e80_bf16_gt', P._mfma(1, 2, 320, 32, E, True, bf16=True), P.ATOMIC)),
]


@pytest.mark.parametrize('entry,case', E80_CASES, ids=lambda x: x.name if isinstance(x, P.Case) else x)
def test_e80_entry_ignores_what_its_buffers_held(entry, case):
    P.test_entry_ignores_what_its_buffers_held(entry, case)


# ---- layers ----

def _layer(kind):
    from naive_gpt import layers
    cls = layers.SparseVanillaAttentionV2 if kind == 'vanilla' else layers.SparseRotaryAttentionV2
    return cls(d_head=E, d_codeword=8, n_codewords=16, p_dropout=0.0).cuda()


@pytest.mark.parametrize('kind', ['vanilla', 'rotary'])
def test_e80_layer_runs_on_the_matrix_cores_and_equals_separate_operators(kind, monkeypatch):
    from naive_gpt import ext
    torch.manual_seed(0)
    attn = _layer(kind)
    N, S, H = 2, 256, 16
    q, k, v, w = [torch.randn([N, S, H, E], device='cuda') for _ in range(4)]

    def run(mfma):
        if not mfma:
            monkeypatch.setattr(ext, 'attention_mfma_supported', lambda *a: False)
            monkeypatch.setattr(ext, 'fused_attention_supported', lambda *a: False)
        ext.reset_paths()
        qi, ki, vi = [t.clone().requires_grad_(True) for t in (q, k, v)]
        y = attn(qi, ki, vi, attn_mask=None)
        (y * w).sum().backward()
        paths = ext.paths_taken('attention')
        monkeypatch.undo()
        return (y.detach(), qi.grad, ki.grad, vi.grad), paths

    fast, paths = run(True)
    assert set(paths) == {('attention', 'mfma')}, paths
    separate, _ = run(False)
    for a, b, name in zip(fast, separate, ['y', 'grad_q', 'grad_k', 'grad_v']):
        assert torch.allclose(a, b, rtol=1e-3, atol=2e-4 * b.abs().max().item()), name


def test_e80_bf16_layer_equals_the_fp32_layer_on_the_widened_values():
    torch.manual_seed(0)
    attn = _layer('vanilla')
    N, S, H = 2, 256, 16
    q, k, v, w = [torch.randn([N, S, H, E], device='cuda').bfloat16() for _ in range(4)]
    got_attn, want_attn = attn._sparse_attn(q, k), attn._sparse_attn(q.float(), k.float())
    assert got_attn[0] == want_attn[0] == 'mfma'
    assert torch.equal(got_attn[2], want_attn[2])

    def run(cast):
        qi, ki, vi = [cast(t).clone().requires_grad_(True) for t in (q, k, v)]
        y = attn(qi, ki, vi, attn_mask=None)
        (y * cast(w)).sum().backward()
        return [t.float() for t in (y.detach(), qi.grad, ki.grad, vi.grad)]

    got, want = run(lambda t: t), run(lambda t: t.float())
    for a, b, name in zip(got, want, ['y', 'grad_q', 'grad_k', 'grad_v']):
        assert torch.allclose(a, b, rtol=2e-2, atol=2e-2 * b.abs().max().item()), name


@pytest.mark.parametrize('pair', [False, True])
def test_e80_armed_step_takes_the_fused_pq_loss(pair, monkeypatch):
    from naive_gpt import ext
    from naive_gpt.layers.sparse import attention as A
    torch.manual_seed(0)
    attn = _layer('vanilla')
    N, S, H = 2, 256, 16
    q, k, v, w = [torch.randn([N, S, H, E], device='cuda') for _ in range(4)]

    def run(fused):
        if not fused:
            monkeypatch.setattr(ext, 'pq_loss_supported', lambda *a: False)
        attn.zero_grad()
        attn.arm()
        ext.reset_paths()
        if pair:
            qk = torch.stack([q, k]).requires_grad_(True)
            qi, ki = qk[0], qk[1]
        else:
            qi, ki = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
        vi = v.clone().requires_grad_(True)
        y = attn(qi, ki, vi, attn_mask=None)
        ((y * w).sum() + 3.0 * attn.loss).backward()
        paths = ext.paths_taken('pq_loss_forward')
        grads = (qk.grad[0], qk.grad[1]) if pair else (qi.grad, ki.grad)
        out = (attn.loss.detach().clone(), y.detach(), *grads, vi.grad, attn.quantizer.weight.grad.clone())
        monkeypatch.undo()
        return out, paths

    assert A.FOLD_PQ_LOSS
    fused, paths = run(True)
    assert paths == {('pq_loss_forward', 'pair' if pair else 'each'): 1}, paths
    composed, _ = run(False)
    for a, b, name in zip(fused, composed, ['loss', 'y', 'grad_q', 'grad_k', 'grad_v', 'grad_table']):
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-3 * b.abs().max().item()), name


def test_e80_fullsize_opt_2_7b_attention_against_a_dense_fp64_restatement():
    """N = 1, S = 2048, H = 32, d_head 80 with lookup's indices: a few (head, row) slices of y
    against y_i = sum_p exp(clamp(scale q_i . k_j)) v_j / sum_p exp(..) in fp64."""
    from naive_gpt import ext
    torch.manual_seed(1)
    attn = _layer('vanilla')
    N, S, H = 1, 2048, 32
    q, k, v = [torch.randn([N, S, H, E], device='cuda') for _ in range(3)]
    ext.reset_paths()
    with torch.no_grad():
        y = attn(q, k, v, attn_mask=None)
        kind, _, csr = attn._get_attn(q, k, None)[:3]
    assert kind == 'mfma' and ('attention', 'mfma') in ext.paths_taken('attention')
    Z = csr.size(-1) // S
    csr = csr.view(N * H, S, Z).cpu()
    scale = E ** -0.5
    qd, kd, vd = (t.double().cpu() for t in (q, k, v))
    yc = y.double().cpu().reshape(N * H, E, S)     # the reference's [N * H, E, S] buffer as [N, S, H, E]
    for h in (0, 13, 31):
        for i in (0, 1, 777, 2047):
            cols = csr[h, i].long()
            cols = cols[cols <= i]
            s = (kd[0, cols, h] @ qd[0, i, h] * scale).clamp(-CLAMP, CLAMP)
            p = s.exp()
            want = (p[:, None] * vd[0, cols, h]).sum(0) / max(1e-9, float(p.sum()))
            got = yc[h, :, i]
            assert torch.allclose(got, want, rtol=1e-3, atol=1e-4 * float(want.abs().max())), (h, i)


# ---- the fused PQ loss at M = 10 ----

def test_pq_loss_at_ten_subspaces_matches_the_composed_loss(monkeypatch):
    from naive_gpt import ext
    torch.manual_seed(0)
    quant = _layer('vanilla').quantizer                    # d_head 80 / d_codeword 8: M = 10
    table = quant.weight
    assert tuple(table.shape) == (10, 16, 8)
    # large enough that every kernel's grid is capped (the rounded grid stride)
    z = torch.randn([4, 2048, 16, E], device='cuda')
    assert ext.pq_loss_supported(z, table.detach())
    loss, codes = ext.pq_loss_forward(z, table.detach(), want_codes=True)
    assert torch.equal(codes, ext.pq_encode_heads(z, table.detach()))

    def grads(fused):
        if not fused:
            monkeypatch.setattr(ext, 'pq_loss_supported', lambda *a: False)
        zi = z.clone().requires_grad_(True)
        quant.zero_grad()
        out = quant.train_loss(zi)
        out.backward()
        monkeypatch.undo()
        return out.detach(), zi.grad, table.grad.clone()

    fused, composed = grads(True), grads(False)
    assert torch.allclose(loss, composed[0], rtol=1e-3)
    for a, b, name in zip(fused, composed, ['loss', 'grad_z', 'grad_table']):
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-3 * b.abs().max().item()), name
    # `parts`: q and k back to back in one buffer, one pass (spt_pq_loss_*_parts)
    qk = torch.randn([2, 2, 512, 16, E], device='cuda')
    lp, cq, ck = ext.pq_loss_forward_pair(qk[0], qk[1], table.detach())
    lq, cq1 = ext.pq_loss_forward(qk[0].contiguous(), table.detach(), want_codes=True)
    lk, ck1 = ext.pq_loss_forward(qk[1].contiguous(), table.detach(), want_codes=True)
    assert torch.equal(cq, cq1) and torch.equal(ck, ck1)
    assert torch.allclose(lp, lq + lk, rtol=1e-5)
