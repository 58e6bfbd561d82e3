"""GPU tier: bf16 routed FFNs on the grouped matrix-core path (spt_grouped_gemm_bf16,
spt_grouped_gemm_wgrad_bf16, spt_rows_combine_bf16, spt_swiglu_*_bf16).

Contract (include/spt_hip.h): fp32 accumulation of the exact products of the stored bf16 values,
rounded once when stored.  The kernels are checked against fp64 on the WIDENED bf16 values with the
bar 1e-3 max|want| + 2^-8 |want|, and against the fp32 kernels run on the same widened values (they
may differ by the bf16 store's rounding alone).  The layers are checked against fp64 and against the
bf16 per-block loop, the trainable path over two AdamW steps, and a captured HIP graph against eager."""
import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _bar(got, want):
    """|got - want| <= 1e-3 max|want| + 2^-8 |want| element by element"""
    got, want = got.double(), want.double()
    tol = 1e-3 * want.abs().max().item() + 2.0 ** -8 * want.abs()
    return bool(((got - want).abs() <= tol).all())


def _one_rounding(got, fp32):
    """the bf16 result is the fp32 kernel's value rounded once: within half an ulp (2^-8 relative)
    of it, plus the fp32 kernel's own split error"""
    got, fp32 = got.double(), fp32.double()
    tol = 2.0 ** -8 * fp32.abs() + 1e-4 * fp32.abs().max().item()
    return bool(((got - fp32).abs() <= tol).all())


def _layer_close(got, want, frac=1e-2):
    """bf16 tolerance of a layer (several stores in a row): frac of scale + 2^-6 relative"""
    got, want = got.double(), want.double()
    tol = frac * want.abs().max().item() + 2.0 ** -6 * want.abs()
    return bool(((got - want).abs() <= tol).all())


def _act64(act, s):
    if act == 0:
        return s.clamp_min(0)
    if act == 1:
        return 0.5 * s * (1 + torch.erf(s / 2 ** 0.5))
    return s * torch.sigmoid(s)


# ragged buckets, with empty ones (first, middle, last)
SIZES = [0, 97, 300, 0, 1, 129, 0]


def _case(layout, gather, seed):
    """operands of one grouped product (widened bf16 values) and its fp64 per-row formula"""
    gen = torch.Generator().manual_seed(seed)
    G, P = len(SIZES), sum(SIZES)
    offsets = torch.tensor([0] + torch.tensor(SIZES).cumsum(0).tolist(), dtype=torch.int32)
    if layout == 'fc1':           # W1 [G n, k]: (n, k, n k, k, 1)
        n, k = 192, 256
        w = torch.randn([G * n, k], generator=gen)
        view = (n, k, n * k, k, 1)
    elif layout == 'fc2':         # W2 [n, G k]: (n, k, k, G k, 1)
        n, k = 256, 192
        w = torch.randn([n, G * k], generator=gen)
        view = (n, k, k, G * k, 1)
    elif layout == 'fc1_dx':      # the swapped view of fc1 (n-contiguous): (d, bs, bs d, 1, d)
        n, k = 256, 192
        w = torch.randn([G * k, n], generator=gen)
        view = (n, k, k * n, 1, n)
    else:                         # fc2_dx: (bs, d, bs, 1, G bs)
        n, k = 192, 256
        w = torch.randn([k, G * n], generator=gen)
        view = (n, k, n, 1, G * n)
    T = 400
    a = torch.randn([T if gather else P, k], generator=gen)
    src = torch.randint(0, T, [P], generator=gen, dtype=torch.int32) if gather else None
    a, w = a.to(BF), (w / k ** 0.5).to(BF)
    return dict(offsets=offsets, view=view, a=a, w=w, gather=src, gen=gen, G=G, P=P, n=n, k=k)


def _ref_pre(c, bias, rowscale):
    """fp64 rowscale * (a[src] W_g^T + bias_g) over the rows, and sum_k |a w| (the accumulation bound)"""
    n, k, gs, ldn, ldk = c['view']
    a64, wflat = c['a'].double(), c['w'].double().reshape(-1)
    out = torch.zeros([c['P'], n], dtype=torch.float64)
    mag = torch.zeros([c['P'], n], dtype=torch.float64)
    offs = c['offsets'].tolist()
    for g in range(c['G']):
        rows = torch.arange(offs[g], offs[g + 1])
        if rows.numel() == 0:
            continue
        idx = g * gs + torch.arange(n)[:, None] * ldn + torch.arange(k)[None, :] * ldk
        wg = wflat[idx]                                      # [n, k]
        src = c['gather'].long()[rows] if c['gather'] is not None else rows
        ar = a64[src]
        v = ar @ wg.T
        if bias is not None:
            v = v + bias.double()[g]
        mag[rows] = ar.abs() @ wg.abs().T
        if rowscale is not None:
            v = v * rowscale.double()[rows][:, None]
            mag[rows] = mag[rows] * rowscale.double()[rows][:, None]
        out[rows] = v
    return out, mag


def _cuda(t):
    return t.cuda() if t is not None else None


@pytest.mark.parametrize('layout', ['fc1', 'fc2', 'fc1_dx', 'fc2_dx'])
@pytest.mark.parametrize('epi', ['plain', 'relu', 'gelu', 'silu'])
@pytest.mark.parametrize('extras', [False, True])
def test_forward_kernel_against_fp64_and_fp32_kernel(layout, epi, extras):
    """ragged / empty groups, gather, rowscale and bias (extras), every epilogue, both weight orientations"""
    from naive_gpt import ext
    c = _case(layout, gather=extras, seed=31 * len(layout) + 7 * len(epi) + int(extras))
    n, k, gs, ldn, ldk = c['view']
    bias = torch.randn([c['G'], n], generator=c['gen']).to(BF) if extras else None
    rowscale = torch.rand([c['P']], generator=c['gen']) + 0.5 if extras else None
    pre, _ = _ref_pre(c, bias, rowscale)
    args = (_cuda(c['a']), _cuda(c['w']), _cuda(c['offsets']), c['G'], n, k, gs, ldn, ldk)
    kw = dict(n_rows=c['P'], gather=_cuda(c['gather']), bias=_cuda(bias), rowscale=_cuda(rowscale))
    if epi == 'plain':
        out = torch.full([c['P'], n], float('nan'), dtype=BF, device='cuda')     # written whole
        got = ext.grouped_gemm_bf16(*args, out=out, **kw)
        assert got.data_ptr() == out.data_ptr() and got.dtype == BF
        want = pre
        fp32 = ext.grouped_gemm(c['a'].float().cuda(), c['w'].float().cuda(), _cuda(c['offsets']), c['G'], n, k,
                                gs, ldn, ldk, gather=_cuda(c['gather']),
                                bias=bias.float().cuda() if extras else None, rowscale=_cuda(rowscale))
        assert _one_rounding(got.cpu(), fp32.cpu())
        # the simple entry dispatches on dtype
        again = ext.grouped_gemm(*args, **kw)
        assert torch.equal(again, got)
    else:
        act = {'relu': ext.ACT_RELU, 'gelu': ext.ACT_GELU, 'silu': ext.ACT_SILU}[epi]
        got, preact = ext.grouped_gemm_bf16(*args, epilogue=ext.EPI_ACT, activation=act, keep_preact=True, **kw)
        want = _act64(act, pre)
        assert _bar(preact.cpu(), pre)
    assert torch.isfinite(got).all()
    assert _bar(got.cpu(), want)


@pytest.mark.parametrize('epi', ['relu', 'gelu'])
def test_activation_masks_follow_the_fp64_sign(epi):
    """where |pre| exceeds the accumulation bound the stored activation has the fp64 pre-activation's
    sign (ReLU: h > 0 exactly where pre > 0)"""
    from naive_gpt import ext
    c = _case('fc1', gather=True, seed=11)
    n, k, gs, ldn, ldk = c['view']
    act = ext.ACT_RELU if epi == 'relu' else ext.ACT_GELU
    pre, mag = _ref_pre(c, None, None)
    h, _ = ext.grouped_gemm_bf16(_cuda(c['a']), _cuda(c['w']), _cuda(c['offsets']), c['G'], n, k, gs, ldn, ldk,
                                 n_rows=c['P'], gather=_cuda(c['gather']), epilogue=ext.EPI_ACT, activation=act)
    h = h.cpu().double()
    clear = pre.abs() > 2.0 ** -20 * mag + 1e-30         # fp32 accumulation of k exact products
    assert clear.float().mean() > 0.99
    if epi == 'relu':
        assert torch.equal((h > 0)[clear], (pre > 0)[clear])
    else:
        assert torch.equal(torch.sign(h)[clear & (h != 0)], torch.sign(pre)[clear & (h != 0)])


def test_dact_epilogue_against_fp64():
    from naive_gpt import ext
    c = _case('fc2_dx', gather=True, seed=5)
    n, k, gs, ldn, ldk = c['view']
    pre, _ = _ref_pre(c, None, None)
    s = torch.randn([c['P'], n], generator=c['gen']).to(BF)
    got = ext.grouped_gemm_bf16(_cuda(c['a']), _cuda(c['w']), _cuda(c['offsets']), c['G'], n, k, gs, ldn, ldk,
                                n_rows=c['P'], gather=_cuda(c['gather']), epilogue=ext.EPI_DACT,
                                activation=ext.ACT_GELU, s_in=_cuda(s))
    s64 = s.double().requires_grad_(True)
    d, = torch.autograd.grad(_act64(1, s64), s64, torch.ones_like(s64))
    assert _bar(got.cpu(), pre * d)


def test_mixed_dtypes_are_refused():
    from naive_gpt import ext
    c = _case('fc1', gather=False, seed=3)
    n, k, gs, ldn, ldk = c['view']
    with pytest.raises(RuntimeError, match='mixed dtypes'):
        ext.grouped_gemm(_cuda(c['a']), c['w'].float().cuda(), _cuda(c['offsets']), c['G'], n, k, gs, ldn, ldk)
    with pytest.raises(RuntimeError, match='mixed dtypes'):
        ext.grouped_gemm_wgrad(torch.zeros([c['P'], n], device='cuda'), _cuda(c['a']), _cuda(c['offsets']),
                               c['view'], c['P'])


# ------------------------------------------------------------------ weight gradients

def _ref_wgrad(grad, a, offsets, view, gather_g, gather_a, rowscale, size):
    n, k, gs, ldn, _ = view
    out = torch.zeros([size], dtype=torch.float64)
    dbias = torch.zeros([len(offsets) - 1, n], dtype=torch.float64)
    grad, a = grad.double(), a.double()
    for g in range(len(offsets) - 1):
        rows = torch.arange(offsets[g], offsets[g + 1])
        sg = gather_g.long()[rows] if gather_g is not None else rows
        sa = gather_a.long()[rows] if gather_a is not None else rows
        gr = grad[sg]
        if rowscale is not None:
            gr = gr * rowscale.double()[rows][:, None]
        idx = g * gs + torch.arange(n)[:, None] * ldn + torch.arange(k)[None, :]
        out[idx.reshape(-1)] = (gr.T @ a[sa]).reshape(-1)
        dbias[g] = gr.sum(0)
    return out, dbias


@pytest.mark.parametrize('gathers', ['none', 'g', 'a', 'both'])
@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('layout', ['fc1', 'fc2'])
def test_wgrad_matches_fp64_per_group_formula(gathers, scaled, layout):
    from naive_gpt import ext
    gen = torch.Generator().manual_seed(17)
    sizes = [37, 0, 1, 2113, 260, 0]
    P, G = sum(sizes), len(sizes)
    offsets = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32)
    if layout == 'fc1':
        n, k = 196, 100
        view, size = (n, k, n * k, k, 1), G * n * k
    else:
        n, k = 132, 64
        view, size = (n, k, k, G * k, 1), n * G * k
    T = 700
    grad = torch.randn([T if gathers in ('g', 'both') else P, n], generator=gen).to(BF)
    a = torch.randn([T if gathers in ('a', 'both') else P, k], generator=gen).to(BF)
    gather_g = torch.randint(0, T, [P], generator=gen, dtype=torch.int32) if gathers in ('g', 'both') else None
    gather_a = torch.randint(0, T, [P], generator=gen, dtype=torch.int32) if gathers in ('a', 'both') else None
    rowscale = torch.rand([P], generator=gen) + 0.5 if scaled else None
    want, want_bias = _ref_wgrad(grad, a, offsets.tolist(), view, gather_g, gather_a, rowscale, size)
    out = torch.full([size], float('nan'), dtype=BF, device='cuda')              # written whole
    kw = dict(gather_grad=_cuda(gather_g), gather_a=_cuda(gather_a), rowscale=_cuda(rowscale), want_bias=True)
    got, dbias = ext.grouped_gemm_wgrad(grad.cuda(), a.cuda(), offsets.cuda(), view, P, out=out, **kw)
    assert got.dtype == dbias.dtype == BF
    assert _bar(got.cpu(), want) and _bar(dbias.cpu(), want_bias.reshape(-1).view(G, n))
    # empty groups: zeros
    assert (dbias[1] == 0).all() and (dbias[5] == 0).all()
    # against the fp32 kernel on the widened values
    got32, db32 = ext.grouped_gemm_wgrad(grad.float().cuda(), a.float().cuda(), offsets.cuda(), view, P, **kw)
    assert _one_rounding(got.cpu(), got32.cpu()) and _one_rounding(dbias.cpu(), db32.cpu())
    # two calls: bitwise equal
    again, dbias2 = ext.grouped_gemm_wgrad(grad.cuda(), a.cuda(), offsets.cuda(), view, P, **kw)
    assert torch.equal(again, got) and torch.equal(dbias2, dbias)


def test_rows_combine_and_swiglu_bf16():
    from naive_gpt import ext
    gen = torch.Generator().manual_seed(2)
    T, k, d = 300, 3, 192
    rows = torch.randn([T * k, d], generator=gen).to(BF)
    pos = torch.randperm(T * k, generator=gen).view(T, k).int()
    bias = torch.randn([d], generator=gen).to(BF)
    got = ext.rows_combine(rows.cuda(), pos.cuda(), bias=bias.cuda())
    want = bias.double() + rows.double()[pos.long()].sum(1)
    assert got.dtype == BF and _one_rounding(got.cpu(), want)
    g, s, dh = [torch.randn([64, 256], generator=gen).to(BF) for _ in range(3)]
    h = ext.swiglu_forward_bf16(g.cuda(), s.cuda())
    g64 = g.double().requires_grad_(True)
    s64 = s.double().requires_grad_(True)
    h64 = g64 * torch.sigmoid(g64) * s64
    assert _one_rounding(h.cpu(), h64.detach())
    dg, ds = ext.swiglu_backward_bf16(dh.cuda(), g.cuda(), s.cuda())
    dg64, ds64 = torch.autograd.grad(h64, (g64, s64), dh.double())
    assert _one_rounding(dg.cpu(), dg64) and _one_rounding(ds.cpu(), ds64)


# ------------------------------------------------------------------ bucketing of bf16 probabilities

def test_bucket_assignment_matches_topk_except_exact_ties():
    """spt_route_topk on widened bf16 probabilities picks torch.topk's set wherever the k-th and
    (k+1)-th probabilities differ; on an exact tie it takes the lower block index"""
    from naive_gpt.layers.sparse import grouped
    gen = torch.Generator().manual_seed(4)
    T, nb, k = 4096, 8, 4
    prob = torch.sigmoid(torch.randn([T, nb], generator=gen) * 0.05).to(BF)   # many exact ties
    bk = grouped.make_buckets(prob.cuda().float(), k=k)
    chosen = torch.zeros([T, nb], dtype=torch.bool)
    chosen[bk.token_long.cpu(), bk.block.cpu()] = True
    assert (chosen.sum(1) == k).all()
    top = torch.sort(prob.float(), dim=-1, descending=True).values
    tied = top[:, k - 1] == top[:, k]
    assert tied.any() and (~tied).any()
    ref = torch.zeros([T, nb], dtype=torch.bool)
    ref.scatter_(1, torch.topk(prob.float(), k, dim=-1).indices, True)
    assert torch.equal(chosen[~tied], ref[~tied])
    # ties: every block above the k-th value, then the tied ones in ascending block index
    kth = top[:, k - 1:k]
    above = prob.float() > kth
    at = prob.float() == kth
    need = k - above.sum(1, keepdim=True)
    rule = above | (at & (at.int().cumsum(1) <= need))
    assert torch.equal(chosen, rule)


# ------------------------------------------------------------------ the layers

def _layer(kind, d, dff, bs, act=None):
    from naive_gpt import layers
    if kind == 'opt':
        m = layers.RoutedFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=act or nn.ReLU())
        k = m.n_blocks // 2
    else:
        m = layers.RoutedLLaMaFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=act or nn.SiLU())
        k = m.n_blocks // 4
    return m.cuda().to(BF), k


def _untied_tokens(m, k, n_tokens, d, seed):
    """n_tokens inputs whose bf16 router probabilities do not tie at the top-k boundary (the loop's
    torch.topk and the kernel's bucketing then pick the same blocks)"""
    gen = torch.Generator().manual_seed(seed)
    pool = torch.randn([2 * n_tokens, d], generator=gen).cuda().to(BF)
    with torch.no_grad():
        top = torch.sort(m.router(pool).float(), dim=-1, descending=True).values
    x = pool[top[:, k - 1] > top[:, k]][:n_tokens]
    assert x.size(0) == n_tokens
    return x.contiguous()


def _fp64_layer(m, kind, x, k):
    """the layer in fp64 on the bf16 values, with the kernels' own bucket assignment"""
    from naive_gpt.layers.sparse import grouped
    with torch.no_grad():
        bk = grouped.make_buckets(m.router(x).float(), k=k)
    x64 = x.double().requires_grad_(True)
    m64 = copy.deepcopy(m).double()
    bs = m.block_size
    offsets = bk.offsets.tolist()
    y = torch.zeros_like(x64)
    for g in range(m.n_blocks):
        tok = bk.token_long[offsets[g]:offsets[g + 1]]
        if tok.numel() == 0:
            continue
        blk = slice(g * bs, (g + 1) * bs)
        xr = x64[tok]
        if kind == 'opt':
            h = m64.activation(xr @ m64.fc1.weight[blk].T + m64.fc1.bias[blk])
            ys = h @ m64.fc2.weight[:, blk].T
        else:
            h = m64.activation(xr @ m64.gate.weight[blk].T) * (xr @ m64.side.weight[blk].T)
            ys = h @ m64.down.weight[:, blk].T
        y = y.index_add(0, tok, ys)
    if kind == 'opt':
        y = y + m64.fc2.bias
    return y, x64, m64


SHAPES = {'configs2': (1024, 4096, 1024, 2048), 'ragged_small': (192, 768, 192, 333)}


@pytest.mark.parametrize('kind', ['opt', 'llama'])
@pytest.mark.parametrize('shape', ['configs2', 'ragged_small'])
def test_frozen_layers_take_the_bf16_grouped_path(kind, shape):
    from naive_gpt import ext
    torch.manual_seed(21)
    d, dff, bs, T = SHAPES[shape]
    m, k = _layer(kind, d, dff, bs)
    for p in m.parameters():
        p.requires_grad_(False)
    x = _untied_tokens(m, k, T, d, 8).requires_grad_(True)
    w = torch.randn([T, d], device='cuda').to(BF)
    ext.reset_paths()
    y = m(x)
    (y.float() * w.float()).sum().backward()
    assert ext.paths_taken('routed_ffn_plain') == {('routed_ffn_plain', 'grouped_bf16'): 1}
    assert ext.paths_taken('route_topk') == {('route_topk', 'kernel'): 1}
    assert ext.paths_taken('grouped_gemm').get(('grouped_gemm', 'bf16'), 0) >= 3
    assert y.dtype == x.grad.dtype == BF
    # fp64 on the bf16 values, the kernels' own bucket assignment
    y64, x64, _ = _fp64_layer(m, kind, x.detach(), k)
    (y64 * w.double()).sum().backward()
    assert _layer_close(y, y64) and _layer_close(x.grad, x64.grad)
    # the bf16 loop (torch.topk: no ties among these tokens)
    x_loop = x.detach().clone().requires_grad_(True)
    for p in m.parameters():
        p.requires_grad_(True)
    ext.reset_paths()
    y_loop = m(x_loop)
    assert ext.paths_taken('routed_ffn_plain') == {('routed_ffn_plain', 'torch_loop'): 1}
    (y_loop.float() * w.float()).sum().backward()
    assert _layer_close(y, y_loop) and _layer_close(x.grad, x_loop.grad)


@pytest.fixture
def trainable(monkeypatch):
    from naive_gpt.layers.sparse import grouped
    monkeypatch.setattr(grouped, 'TRAINABLE_WEIGHTS', True)
    return grouped


@pytest.mark.parametrize('kind,act', [('opt', nn.ReLU()), ('opt', nn.GELU()), ('llama', nn.SiLU())])
@pytest.mark.parametrize('shape', ['configs2', 'ragged_small'])
def test_trainable_layers_against_fp64(kind, act, shape, trainable):
    from naive_gpt import ext
    torch.manual_seed(5)
    d, dff, bs, T = SHAPES[shape]
    m, k = _layer(kind, d, dff, bs, act)
    x = _untied_tokens(m, k, T, d, 3).requires_grad_(True)
    w = torch.randn([T, d], device='cuda').to(BF)
    ext.reset_paths()
    y = m(x)
    (y.float() * w.float()).sum().backward()
    assert ext.paths_taken('routed_ffn_plain') == {('routed_ffn_plain', 'grouped_trainable_bf16'): 1}
    y64, x64, m64 = _fp64_layer(m, kind, x.detach(), k)
    (y64 * w.double()).sum().backward()
    assert _layer_close(y, y64) and _layer_close(x.grad, x64.grad)
    for (name, p), p64 in zip(m.named_parameters(), m64.parameters()):
        if name.startswith('router'):
            assert p.grad is None
        else:
            assert p.grad.dtype == BF, name
            assert _layer_close(p.grad, p64.grad), name


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_two_adamw_steps_match_the_bf16_loop(kind, trainable, monkeypatch):
    """after two AdamW steps the weights of the grouped path and of the bf16 loop differ by at most
    15 % of the loop's own update (bf16 rounding of the gradients and of every stored weight)"""
    from naive_gpt import ext
    torch.manual_seed(9)
    d, dff, bs, T = 256, 1024, 128, 1024
    m, k = _layer(kind, d, dff, bs)
    x = _untied_tokens(m, k, T, d, 1)
    w = torch.randn([T, d], device='cuda').to(BF)
    ref = copy.deepcopy(m)
    start = [p.detach().clone() for p in m.parameters()]
    for model, on in ((m, True), (ref, False)):
        monkeypatch.setattr(trainable, 'TRAINABLE_WEIGHTS', on)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-2, eps=1e-3)
        ext.reset_paths()
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            (model(x).float() * w.float()).sum().backward()
            opt.step()
        want = 'grouped_trainable_bf16' if on else 'torch_loop'
        assert ext.paths_taken('routed_ffn_plain') == {('routed_ffn_plain', want): 2}
    for (name, p), p_loop, p0 in zip(m.named_parameters(), ref.parameters(), start):
        step = (p_loop.float() - p0.float()).norm().item()
        assert (p.float() - p_loop.float()).norm().item() <= 0.15 * step + 1e-6, name


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_graph_capture_replays_bitwise(kind, trainable):
    torch.manual_seed(13)
    d, dff, bs, T = 256, 1024, 128, 512
    m, _ = _layer(kind, d, dff, bs)
    x = torch.randn([T, d], device='cuda').to(BF).requires_grad_(True)
    w = torch.randn([T, d], device='cuda').to(BF)
    params = list(m.parameters())

    def step():
        x.grad = None
        for p in params:
            p.grad = None
        y = m(x)
        (y * w).sum().backward()
        return y

    y_eager = step().detach().clone()
    grads_eager = [x.grad.clone()] + [p.grad.clone() if p.grad is not None else None for p in params]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    x.grad = None
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_static = m(x)
        (y_static * w).sum().backward()
    with torch.no_grad():
        y_static.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_static, y_eager)
    for g, ge in zip([x.grad] + [p.grad for p in params], grads_eager):
        assert (g is None) == (ge is None)
        if g is not None:
            assert torch.equal(g, ge)
    # The same graph on new contents of its buffers: new tokens, a new upstream gradient, and every
    # trained parameter nudged in place, as the in-graph optimiser moves it between two replays.
    with torch.no_grad():
        x.copy_(torch.randn([T, d], device='cuda').to(BF))
        w.copy_(torch.randn([T, d], device='cuda').to(BF))
        for p in params:
            if p.requires_grad:
                p.add_((0.01 * torch.randn(p.shape, device='cuda')).to(p.dtype))
    graph.replay()
    torch.cuda.synchronize()
    y_replay = y_static.detach().clone()
    grads_replay = [None if g is None else g.clone() for g in [x.grad] + [p.grad for p in params]]
    y_new = step().detach().clone()
    assert not torch.equal(y_new, y_eager), 'the new contents changed nothing'
    assert torch.equal(y_replay, y_new)
    for i, (g, ge) in enumerate(zip(grads_replay, [x.grad] + [p.grad for p in params])):
        assert (g is None) == (ge is None)
        if g is not None:
            assert torch.equal(g, ge), 'gradient %d' % i


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_lora_routed_variants_keep_their_fp32_gate(kind):
    """the bf16 grouped path is the plain routed FFNs' only: a bf16 LoRA routed FFN (frozen base weights
    by construction) still takes its per-block torch loop, forward and backward"""
    from naive_gpt import ext, layers
    torch.manual_seed(4)
    d, dff, bs, r = 128, 512, 128, 8
    if kind == 'opt':
        m = layers.LoRARoutedFFN(d_lora=r, block_size=bs, d_model=d, d_feedforward=dff, activation=nn.ReLU())
    else:
        m = layers.LoRARoutedLLaMaFFN(d_lora=r, block_size=bs, d_model=d, d_feedforward=dff,
                                      activation=nn.SiLU())
    m = m.cuda().to(BF)
    x = torch.randn([300, d], device='cuda').to(BF).requires_grad_(True)
    ext.reset_paths()
    y = m(x)
    y.float().sum().backward()
    assert ext.paths_taken('routed_ffn') == {('routed_ffn', 'torch_loop'): 1}
    assert ext.paths_taken('routed_ffn_plain') == {}
    assert y.dtype == BF and torch.isfinite(y).all() and torch.isfinite(x.grad).all()
