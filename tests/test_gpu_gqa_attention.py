"""Sparse attention with grouped key/value heads (GQA / MQA) on the GPU.

The arithmetic contract needs no measured tolerance:

* forward y, row_sum, bounds and grad_q of a grouped call are the bits of the existing entries on k, v
  repeated per group (`repeat_interleave` along the head axis): same instructions on the same values;
* so are the per-query-head partials of grad_k / grad_v;
* the reduced grad_k / grad_v are those partials summed per group in ascending head order with plain
  fp32 adds, restated here on the CPU;
* against ANOTHER order of the same sum (autograd's reduction of the repeated form) two sums of g
  terms differ by at most 2 (g - 1) 2^-24 sum_i |p_i| per element (each of the g - 1 adds of either
  sum rounds by at most 2^-24 of a partial sum that is at most sum_i |p_i|, to first order; the bound
  is evaluated in fp64 from the partials and given 1e-6 of slack for the second-order terms);
* lookup indices are integers: equal.

K and V are random per kv head, so a wrong head mapping changes bits (checked once below).  The
shapes: N > 1, a group size that is no power of two (6 / 2), MQA (8 / 1), more than one row tile."""
import pytest
import torch

import test_gpu_fused_attention as F
import test_gpu_graph_replay as R
import test_gpu_guard_bands as G
import test_gpu_poisoned_buffers as P

pytestmark = pytest.mark.gpu
CLAMP = 10.0
U = 2.0 ** -24
SHAPES = [(3, 6, 2, 64, 64, 8), (2, 4, 2, 80, 64, 8), (1, 8, 1, 128, 128, 16)]      # (N, H, kv, E, S, Z)


def _repeat(t, heads):
    return t.repeat_interleave(heads // t.size(2), dim=2).contiguous()


def _ordered_sum(parts, kv_heads):
    """[..., H, E] -> [..., kv, E]: ((p_0 + p_1) + p_2) + ... over each group, explicit fp32 adds (CPU)."""
    parts = parts.float().cpu()
    *lead, H, E = parts.shape
    g = H // kv_heads
    p = parts.view(*lead, kv_heads, g, E)
    acc = p[..., 0, :].clone()
    for u in range(1, g):
        acc = acc + p[..., u, :]
    return acc


def _reorder_bound(parts, kv_heads, extra=0.0):
    """(2 (g - 1) + extra) 2^-24 sum_i |p_i| per element, in fp64 (module docstring)."""
    parts = parts.double().cpu()
    *lead, H, E = parts.shape
    g = H // kv_heads
    return (2.0 * (g - 1) + extra) * U * (1.0 + 1e-6) * parts.abs().view(*lead, kv_heads, g, E).sum(-2)


def _within(got, want, bound, name):
    err = (got.double().cpu() - want.double().cpu()).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print('{}: largest |difference| {:.3e}, {:.3f} of its bound'.format(name, float(err.max()), worst))
    assert (err <= bound).all(), '{}: {:.3f} of the reorder bound'.format(name, worst)


def _stats(row_sum, B, S):
    """(row_sum [B, S], the bounds the forward's blocks wrote [B, blocks, 2]) of the forward's buffer"""
    whole = torch.empty(0, dtype=torch.float32, device=row_sum.device).set_(row_sum.untyped_storage())
    slots = (whole.numel() - B * S) // (2 * B)
    blocks = (S + 255) // 256
    return whole[:B * S].view(B, S), whole[B * S:].view(B, slots, 2)[:, :blocks]


def _lookup_pattern(N, H, KV, S, M, gen):
    """Indices as the layer makes them: lookup on random PQ codes, the key codes per KV head."""
    from naive_gpt import ext
    q_c = torch.randint(0, 3, [N * H, S, M], generator=gen, dtype=torch.int32).cuda()
    k_c = torch.randint(0, 3, [N * KV, S, M], generator=gen, dtype=torch.int32).cuda()
    idx = ext.lookup_forward_cuda(torch.empty([8]), q_c, k_c, kv_group=H // KV)
    return idx.flatten(start_dim=1).cpu()


def _attention(idx, q, k, v, gy, gt, compact, **kw):
    """forward + backward through ext on device copies -> dict of results (device tensors)"""
    from naive_gpt import ext
    N, S, H, E = q.shape
    scale = E ** -0.5
    tiles = ext.attention_mfma_prepare(idx.cuda(), S, lookup_pattern=compact)
    assert (tiles.layout == ext.TILES_COMPACT) == compact
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    y, row_sum = ext.attention_mfma_forward(tiles, qd, kd, vd, scale, CLAMP, y_transposed=gt, **kw)
    gyd = (gy.transpose(1, 2).contiguous() if gt else gy).cuda()
    ext.GROUP_PARTS = []
    try:
        gq, gk, gv = ext.attention_mfma_backward(tiles, qd, kd, vd, y, gyd, row_sum, scale, CLAMP, transposed=gt, **kw)
        parts = ext.GROUP_PARTS[0] if ext.GROUP_PARTS else None
    finally:
        ext.GROUP_PARTS = None
    assert not (compact and tiles.broke_promise())
    rs, bounds = _stats(row_sum, N * H, S)
    return dict(y=y, row_sum=rs, bounds=bounds, grad_q=gq, grad_k=gk, grad_v=gv, parts=parts)


@pytest.mark.parametrize('gt', [False, True], ids=['rows', 'transposed'])
@pytest.mark.parametrize('layout', ['full', 'compact'])
@pytest.mark.parametrize('N,H,KV,E,S,Z', SHAPES)
def test_grouped_entries_equal_the_existing_entries_on_repeated_kv(N, H, KV, E, S, Z, layout, gt):
    gen = torch.Generator().manual_seed(100 * E + S + KV)
    if layout == 'compact':
        S, Z = 128, 16                  # lookup-made patterns: S / 8 keys per row
    q = torch.randn([N, S, H, E], generator=gen)
    k, v = torch.randn([N, S, KV, E], generator=gen), torch.randn([N, S, KV, E], generator=gen)
    gy = torch.randn([N * H, S, E], generator=gen)
    idx = _lookup_pattern(N, H, KV, S, E // 8, gen) if layout == 'compact' else F.causal_indices(N * H, S, Z, gen)
    compact = layout == 'compact'
    g = H // KV

    got = _attention(idx, q, k, v, gy, gt, compact, kv_heads=KV)
    want = _attention(idx, q, _repeat(k, H), _repeat(v, H), gy, gt, compact)
    assert want['parts'] is None and got['parts'] is not None
    assert got['grad_k'].shape == got['grad_v'].shape == (N, S, KV, E) and got['grad_q'].shape == (N, S, H, E)
    for name in ('y', 'row_sum', 'bounds', 'grad_q'):
        assert torch.equal(got[name], want[name]), name + ' differs from the existing entry on repeated k, v'
    # the key-owned kernel's partials: one per query head, the existing kernel's bits
    assert torch.equal(got['parts'][0], want['grad_k']), 'grad_k partials'
    assert torch.equal(got['parts'][1], want['grad_v']), 'grad_v partials'
    # the reduced gradients: the fixed-order sum, restated
    assert torch.equal(got['grad_k'].cpu(), _ordered_sum(got['parts'][0], KV)), 'grad_k is not the ordered sum'
    assert torch.equal(got['grad_v'].cpu(), _ordered_sum(got['parts'][1], KV)), 'grad_v is not the ordered sum'
    # another order of the same sum: autograd's reduction of the repeated form
    for i, name in enumerate(('grad_k', 'grad_v')):
        auto = want[name].view(N, S, KV, g, E).sum(3)
        _within(got[name], auto, _reorder_bound(got['parts'][i], KV), '{} {}'.format(name, (N, H, KV, E, S)))
    # kv_heads == heads is today's call
    same = _attention(idx, q, _repeat(k, H), _repeat(v, H), gy, gt, compact, kv_heads=H)
    assert same['parts'] is None
    for name in ('y', 'row_sum', 'bounds', 'grad_q', 'grad_k', 'grad_v'):
        assert torch.equal(same[name], want[name]), name + ' with kv_heads == heads'
    # and the comparison sees a wrong mapping: kv heads dealt round-robin instead of in runs
    if 1 < KV < H:
        wrong = _attention(idx, q, k.repeat(1, 1, g, 1), v.repeat(1, 1, g, 1), gy, gt, compact)
        assert not torch.equal(wrong['y'], got['y'])


def test_binding_refuses_shapes_that_do_not_group():
    from naive_gpt import ext
    q = torch.zeros([2, 64, 6, 64], device='cuda')
    idx = torch.zeros([12, 64 * 8], dtype=torch.int32, device='cuda')
    tiles = ext.attention_mfma_prepare(idx, 64)
    k4, k3 = torch.zeros([2, 64, 4, 64], device='cuda'), torch.zeros([2, 64, 3, 64], device='cuda')
    with pytest.raises(RuntimeError, match='kv_heads must divide'):
        ext.attention_mfma_forward(tiles, q, k4, k4, 0.125, CLAMP, kv_heads=4)
    with pytest.raises(RuntimeError, match='kv_heads, E'):
        ext.attention_mfma_forward(tiles, q, k3, k3, 0.125, CLAMP, kv_heads=2)
    with pytest.raises(RuntimeError, match='same shape'):
        ext.attention_mfma_forward(tiles, q, k3, k3, 0.125, CLAMP)
    with pytest.raises(RuntimeError, match='float32 only'):
        ext.attention_mfma_forward(tiles, q.bfloat16(), k3.bfloat16(), k3.bfloat16(), 0.125, CLAMP, kv_heads=3)
    codes = torch.zeros([12, 128, 8], dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='kv_group'):
        ext.lookup_forward_cuda(torch.empty([8]), codes, codes[:5].contiguous(), kv_group=2)


# ---- lookup ----

# S 128: lookup_rows_kernel; 528 = 16 * 33, the smallest S past 512: lookup_rows_long_kernel; S 1024 at
# Z 512: rows too long for either (their LDS rows exceed 64 KiB): lookup_forward_kernel
@pytest.mark.parametrize('codes', [3, 40], ids=['nibble', 'wide'])
@pytest.mark.parametrize('kv_group', [2, 3, 6])
@pytest.mark.parametrize('S,coeff', [(128, 8), (528, 33), (1024, 2)])
def test_lookup_reads_the_kv_slice(S, coeff, kv_group, codes):
    from naive_gpt import ext
    N, H, M = 2, 6, 8
    KV = H // kv_group
    gen = torch.Generator().manual_seed(S + kv_group)
    q_c = torch.randint(0, codes, [N * H, S, M], generator=gen, dtype=torch.int32).cuda()
    k_c = torch.randint(0, codes, [N * KV, S, M], generator=gen, dtype=torch.int32).cuda()
    config = torch.empty([coeff])
    got = ext.lookup_forward_cuda(config, q_c, k_c, kv_group=kv_group)
    repeated = k_c.view(N, KV, S, M).repeat_interleave(kv_group, dim=1).reshape(N * H, S, M).contiguous()
    want = ext.lookup_forward_cuda(config, q_c, repeated)
    assert got.shape == want.shape == (N * H, S, S // coeff) and got.dtype == torch.int32
    assert torch.equal(got, want)
    assert torch.equal(ext.lookup_forward_cuda(config, q_c, repeated, kv_group=1), want)
    if KV > 1:          # (the codes differ per kv head: another mapping is another pattern)
        other = k_c.view(N, KV, S, M).repeat(1, kv_group, 1, 1).reshape(N * H, S, M).contiguous()
        assert not torch.equal(ext.lookup_forward_cuda(config, q_c, other), want)


# ---- the group sum alone ----

@pytest.mark.parametrize('E', [64, 80, 128])
@pytest.mark.parametrize('g', [2, 3, 8])
def test_head_group_sum_is_the_ordered_sum(g, E):
    """spt_head_group_sum has no wrapper of its own (attention_mfma_backward owns its launch): the C
    entry is called on the current stream.  37 rows of 3 kv heads: a ragged last workgroup."""
    from naive_gpt import ext
    lib = ext.load_library()
    rows, KV = 37, 3
    H = g * KV
    gen = torch.Generator().manual_seed(g * E)
    # magnitudes spread over twelve binades, so that the order of the adds shows in the bits
    parts = (torch.randn([rows, H, E], generator=gen) * torch.exp2(torch.randint(-6, 6, [rows, H, 1], generator=gen).float())).cuda()
    out = torch.full([rows, KV, E], float('nan'), device='cuda')
    rc = lib.spt_head_group_sum(parts.data_ptr(), out.data_ptr(), rows, H, KV, E, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _ordered_sum(parts, KV))
    if g > 2:
        reverse = _ordered_sum(parts.view(rows, KV, g, E).flip(2).reshape(rows, H, E), KV)
        assert not torch.equal(out.cpu(), reverse), 'the inputs cannot tell one order from another'


# ---- the project's three harnesses on the grouped calls ----

def _gqa_case(N, H, KV, E, S, Z, gt, compact):
    """A registry case (test_gpu_poisoned_buffers.Case): forward + backward with kv_heads; its check
    holds every output to the existing entries on the repeated k, v of the SAME build."""
    def build():
        from naive_gpt import ext
        gen = P._gen(7 * S + E + KV)
        B = N * H
        q = torch.randn([N, S, H, E], generator=gen) * 3.0
        k, v = torch.randn([N, S, KV, E], generator=gen), torch.randn([N, S, KV, E], generator=gen)
        gy = torch.randn([B, S, E], generator=gen)
        idx = P._dead_key_indices(B, S, Z, gen, distinct=compact)
        scale = E ** -0.5
        qd, kd, vd, idd = P._dev(q), P._dev(k), P._dev(v), P._dev(idx)
        gyd = P._dev(gy.transpose(1, 2).contiguous() if gt else gy)
        ref = {}

        def call():
            tiles = ext.attention_mfma_prepare(idd, S, lookup_pattern=compact)
            y, row_sum = ext.attention_mfma_forward(tiles, qd, kd, vd, scale, CLAMP, y_transposed=gt, kv_heads=KV)
            gq, gk, gv = ext.attention_mfma_backward(tiles, qd, kd, vd, y, gyd, row_sum, scale, CLAMP,
                                                     transposed=gt, kv_heads=KV)
            return y, row_sum, gq, gk, gv

        def check(outs):
            if not ref:
                want = _attention(idx, q, _repeat(k, H), _repeat(v, H), gy, gt, compact)
                ref.update({n: want[n].cpu() for n in ('y', 'row_sum', 'grad_q')})
                ref['grad_k'], ref['grad_v'] = _ordered_sum(want['grad_k'], KV), _ordered_sum(want['grad_v'], KV)
            for o, name in zip(outs, ('y', 'row_sum', 'grad_q', 'grad_k', 'grad_v')):
                assert torch.equal(o.cpu(), ref[name]), name
            for o, name in zip(outs[3:], ('grad_k', 'grad_v')):
                assert (o[:, S // 2:] == 0).all(), name + ': keys no query attends are not exactly 0'
        return call, check
    return build


def _lookup_case(S, coeff, kv_group):
    def build():
        from naive_gpt import ext
        N, H, M = 2, 6, 8
        KV = H // kv_group
        gen = P._gen(S + kv_group)
        q_c = torch.randint(0, 3, [N * H, S, M], generator=gen, dtype=torch.int32)
        k_c = torch.randint(0, 3, [N * KV, S, M], generator=gen, dtype=torch.int32)
        config = torch.empty([coeff], device='cpu')
        qd, kd = P._dev(q_c), P._dev(k_c)

        def call():
            return ext.lookup_forward_cuda(config, qd, kd, kv_group=kv_group)

        def check(outs):
            want = ext.lookup_forward_cuda(config, q_c.cuda(), k_c.repeat_interleave(kv_group, dim=0).cuda())
            assert torch.equal(outs[0], want)
        return call, check
    return build


# (K and V are g times smaller than q here: a kernel that addressed them through q's view would run
# past them -- between guard bands that is a changed band or a result that differs)
GQA_CASES = [
    ('attention_mfma_backward', P.Case('gqa_6_2_e64_gt', _gqa_case(3, 6, 2, 64, 64, 8, True, False), P.DET)),
    ('attention_mfma_backward', P.Case('gqa_4_2_e80', _gqa_case(2, 4, 2, 80, 64, 8, False, False), P.DET)),
    ('attention_mfma_backward', P.Case('mqa_8_1_e128_compact_gt', _gqa_case(1, 8, 1, 128, 128, 16, True, True), P.DET)),
    ('lookup_forward_cuda', P.Case('kv_group_3_s128', _lookup_case(128, 8, 3), P.DET)),
    ('lookup_forward_cuda', P.Case('kv_group_6_s528', _lookup_case(528, 33, 6), P.DET)),
]
GQA_PARAMS = [pytest.param(entry, c, id='{}-{}'.format(entry, c.name)) for entry, c in GQA_CASES]


@pytest.mark.parametrize('entry,case', GQA_PARAMS)
def test_grouped_entry_ignores_what_its_buffers_held(entry, case):
    """Poisoned outputs, partials and scratch: the same bits."""
    P.test_entry_ignores_what_its_buffers_held(entry, case)


@pytest.mark.parametrize('entry,case', GQA_PARAMS)
def test_grouped_entry_stays_inside_its_buffers(entry, case):
    G.test_entry_stays_inside_its_buffers(entry, case)


@pytest.mark.parametrize('entry,case', GQA_PARAMS)
def test_grouped_entry_replayed_on_new_inputs_equals_eager(entry, case):
    R.test_entry_replayed_on_new_inputs_equals_eager(entry, case)


# ---- layers: the kernel form against SPT_GQA_EXPAND=1 ----

def _layer(kind, E=64):
    from naive_gpt import layers
    cls = layers.SparseVanillaAttentionV2 if kind == 'vanilla' else layers.SparseRotaryAttentionV2
    return cls(d_head=E, d_codeword=8, n_codewords=16, p_dropout=0.0).cuda()


def _layer_run(attn, q, k, v, w, expand, monkeypatch, armed=False):
    from naive_gpt import ext
    monkeypatch.setenv('SPT_GQA_EXPAND', '1' if expand else '0')
    ext.reset_paths(reasons=True)
    attn.zero_grad()
    if armed:
        attn.arm()
    qi, ki, vi = (t.clone().requires_grad_(True) for t in (q, k, v))
    ext.GROUP_PARTS = []
    try:
        y = attn(qi, ki, vi, attn_mask=None)
        loss = (y * w).sum() + (3.0 * attn.loss if armed else 0.0)
        loss.backward()
        parts = list(ext.GROUP_PARTS)
    finally:
        ext.GROUP_PARTS = None
    out = dict(y=y.detach(), grad_q=qi.grad, grad_k=ki.grad, grad_v=vi.grad, parts=parts,
               paths=ext.paths_taken('attention'), loss=attn.loss.detach().clone() if armed else None)
    monkeypatch.undo()
    return out


@pytest.mark.parametrize('kind', ['vanilla', 'rotary'])
def test_layer_kernel_form_against_the_expanded_form(kind, monkeypatch):
    """N 8, H 4, kv 2, S 128 (n * h = 32).  y and grad_q: the same bits.  grad_v: two orders of the
    group's sum, the reorder bound from the kernel form's partials.  grad_k of the vanilla layer
    likewise; the rotary layer's grad_k passes the rotary embedding's adjoint behind the sum,
    cos dk_e +- sin dk_p of an element and its partner p = e +- E / 2: a difference d of the inputs
    becomes at most |d_e| + |d_p|, and the two evaluations round by at most 2 * 2^-24 (|dk_e| + |dk_p|)
    each (two products, one add), with |dk| <= sum_i |p_i|: (2 (g - 1) + 4) 2^-24 (A_e + A_p), A the
    sum of the partials' magnitudes."""
    from naive_gpt import ext
    torch.manual_seed(0)
    attn = _layer(kind)
    N, S, H, KV, E = 8, 128, 4, 2, 64
    q, w = torch.randn([N, S, H, E], device='cuda'), torch.randn([N, S, H, E], device='cuda')
    k, v = torch.randn([N, S, KV, E], device='cuda'), torch.randn([N, S, KV, E], device='cuda')
    kernel = _layer_run(attn, q, k, v, w, False, monkeypatch)
    assert set(kernel['paths']) == {('attention', 'mfma_gqa')}, kernel['paths']
    assert len(kernel['parts']) == 1
    expanded = _layer_run(attn, q, k, v, w, True, monkeypatch)
    assert set(expanded['paths']) == {('attention', 'gqa_expanded'), ('attention', 'mfma')}, expanded['paths']
    assert not expanded['parts']
    assert any('SPT_GQA_EXPAND' in r for r in ext.fallback_reasons('attention', 'gqa_expanded'))
    assert torch.equal(kernel['y'], expanded['y']), 'y'
    assert torch.equal(kernel['grad_q'], expanded['grad_q']), 'grad_q'
    parts = kernel['parts'][0]
    assert kernel['grad_k'].shape == kernel['grad_v'].shape == (N, S, KV, E)
    _within(kernel['grad_v'], expanded['grad_v'], _reorder_bound(parts[1], KV), kind + ' grad_v')
    if kind == 'vanilla':
        bound = _reorder_bound(parts[0], KV)
    else:
        a = _reorder_bound(parts[0], KV, extra=4.0)
        bound = a + a.roll(E // 2, dims=-1)
    _within(kernel['grad_k'], expanded['grad_k'], bound, kind + ' grad_k')


@pytest.mark.parametrize('kind', ['vanilla', 'rotary'])
def test_layer_armed_step_has_one_pq_loss_in_both_forms(kind, monkeypatch):
    """The PQ loss of an armed step is that of q and of the UN-expanded k in either form."""
    from naive_gpt import ext
    torch.manual_seed(1)
    attn = _layer(kind)
    N, S, H, KV, E = 8, 128, 4, 2, 64
    q, w = torch.randn([N, S, H, E], device='cuda'), torch.randn([N, S, H, E], device='cuda')
    k, v = torch.randn([N, S, KV, E], device='cuda'), torch.randn([N, S, KV, E], device='cuda')
    kernel = _layer_run(attn, q, k, v, w, False, monkeypatch, armed=True)
    grad_table = attn.quantizer.weight.grad.clone()
    expanded = _layer_run(attn, q, k, v, w, True, monkeypatch, armed=True)
    assert set(kernel['paths']) == {('attention', 'mfma_gqa')}
    assert torch.equal(kernel['loss'], expanded['loss']), (float(kernel['loss']), float(expanded['loss']))
    assert torch.equal(kernel['y'], expanded['y'])
    # the loss of the un-expanded k, restated
    rot = attn._rotate if kind == 'rotary' else (lambda t: t)
    with torch.no_grad():
        table = attn.quantizer.weight.detach()
        want = ext.pq_loss_forward(rot(q).contiguous(), table) + ext.pq_loss_forward(rot(k).contiguous(), table)
    assert torch.allclose(kernel['loss'], want, rtol=1e-6), (float(kernel['loss']), float(want))
    # and its gradient reached q, k and the codebook in both forms
    for name in ('grad_q', 'grad_k', 'grad_v'):
        a, b = kernel[name], expanded[name]
        assert a.shape == b.shape and torch.isfinite(a).all()
        P._close(a, b, 'armed ' + name, rtol=1e-5)
    P._close(grad_table, attn.quantizer.weight.grad, 'armed grad_table', rtol=1e-5)
    assert float(grad_table.abs().max()) > 0


# ---- model: a 2-layer upgraded GQA LLaMA, one training step in both forms, and resume ----

MODEL = dict(d_model=256, n_heads=4, n_layers=2, max_length=128, vocab_size=512, d_feedforward=1024, p_dropout=0.0,
             n_kv_heads=2)
BATCH = 8


def _tuner(ckpt, gen_seed):
    from naive_gpt import utils
    torch.manual_seed(7)                                # (the upgrade draws the adapters' and the codebooks' values)
    tuner = utils.SparseTuner.from_checkpoint(ckpt, device='cuda')
    gen = P._gen(gen_seed)
    for name, p in tuner.model.named_parameters():
        if name.endswith('lora.right.weight'):          # a fresh adapter is the identity
            p.data.copy_(0.05 * torch.randn(p.shape, generator=gen).cuda())
    return tuner


def test_model_training_step_in_both_forms_and_resume(tmp_path, monkeypatch):
    """The loss of the first step is a function of the forward alone, which is the same bits in both
    forms; the parameters after the step are held to the project's 1e-3 parity bound (of each
    tensor's scale), the step a resumed tuner takes to test_gpu_resume's 1e-5."""
    from naive_gpt import ext, utils
    from naive_gpt.utils import checkpoint
    torch.manual_seed(0)
    ckpt = str(tmp_path / 'llama-gqa-toy.ckpt')
    checkpoint.save_checkpoint(ckpt, MODEL, checkpoint.build_model('llama', MODEL))
    gen = P._gen(41)
    batches = [torch.randint(0, MODEL['vocab_size'], [BATCH, MODEL['max_length'] + 2], generator=gen).cuda()
               for _ in range(2)]
    tuners = []
    try:
        monkeypatch.setenv('SPT_GQA_EXPAND', '0')
        a = _tuner(ckpt, 40)
        tuners.append(a)
        assert a.model.decoders[0].mha.n_kv_heads == 2
        ext.reset_paths(reasons=True)
        loss_a = a.training_step(batches[0])
        assert {k[1] for k in ext.paths_taken('attention')} == {'mfma_gqa'}, ext.paths_taken('attention')
        assert ('qkv_projection', 'separate') in ext.paths_taken('qkv_projection')
        assert any('grouped key/value heads' in r for r in ext.fallback_reasons('qkv_projection', 'separate'))

        monkeypatch.setenv('SPT_GQA_EXPAND', '1')
        b = _tuner(ckpt, 40)
        tuners.append(b)
        ext.reset_paths()
        loss_b = b.training_step(batches[0])
        assert {k[1] for k in ext.paths_taken('attention')} == {'gqa_expanded', 'mfma'}
        monkeypatch.setenv('SPT_GQA_EXPAND', '0')
        print('GQA model step: loss {:.7f} (kernel form) / {:.7f} (expanded form)'.format(float(loss_a), float(loss_b)))
        assert torch.equal(loss_a, loss_b)
        worst = 0.0
        for (n, p), (_, r) in zip(a.model.named_parameters(), b.model.named_parameters()):
            if p.requires_grad:
                worst = max(worst, float((p - r).detach().abs().max() / p.detach().abs().max().clamp_min(1e-30)))
        print('GQA model step: largest parameter difference between the forms {:.3e} of scale'.format(worst))
        for (n, p), (_, r) in zip(a.model.named_parameters(), b.model.named_parameters()):
            if p.requires_grad:
                P._close(r, p, n + ' after the step', rtol=1e-3)

        # resume: the saved kernel-form run and its resumed twin take the same next step
        state = str(tmp_path / 'run.state')
        a.save(state)
        c = utils.SparseTuner.resume(ckpt, state, device='cuda')
        tuners.append(c)
        assert c.model.decoders[1].mha.linear_k.weight.shape == (128, 256)
        la, lc = a.training_step(batches[1]), c.training_step(batches[1])
        P._close(lc, la, 'loss of the resumed step', rtol=1e-5)
        for (n, p), (_, r) in zip(a.model.named_parameters(), c.model.named_parameters()):
            if p.requires_grad:
                P._close(r, p, n + ' after the resumed step', rtol=1e-5)
    finally:
        for t in tuners:
            t.release()
