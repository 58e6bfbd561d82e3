"""GPU tier: the LoRA routed FFNs on bf16 storage (grouped.RoutedLoRAFFNBf16 / RoutedLoRALLaMAFFNBf16 behind
grouped.LORA_BF16) and their kernels: spt_grouped_gemm_bf16_ext (the fp32-a2 / bf16-b2 K extension),
spt_lora_down_bf16 and its grouped form, spt_tall_tn_bf16 and spt_swiglu_backward_dots_bf16.

The kernels are checked against fp64 on the widened bf16 values with the bars of test_gpu_routed_bf16.py; the
layers against an fp64 evaluation of the lora_ffn.py formula (on tokens whose top-k has a clear margin, so
that fp64 and bf16 pick the same blocks) and against the bf16 per-block loop."""
import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _bar(got, want):
    """|got - want| <= 1e-3 max|want| + 2^-8 |want| element by element"""
    got, want = got.double().cpu(), want.double().cpu()
    tol = 1e-3 * want.abs().max().item() + 2.0 ** -8 * want.abs()
    return bool(((got - want).abs() <= tol).all())


def _one_rounding(got, want):
    """a bf16 result within half an ulp (2^-8 relative) of the exact value, plus the fp32 error"""
    got, want = got.double().cpu(), want.double().cpu()
    tol = 2.0 ** -8 * want.abs() + 1e-4 * want.abs().max().item()
    return bool(((got - want).abs() <= tol).all())


def _layer_close(got, want, frac=1e-2):
    """bf16 tolerance of a layer (several stores in a row): frac of scale + 2^-6 relative"""
    got, want = got.double().cpu(), want.double().cpu()
    tol = frac * want.abs().max().item() + 2.0 ** -6 * want.abs()
    return bool(((got - want).abs() <= tol).all())


def _act64(act, s):
    from naive_gpt import ext
    if act == ext.ACT_RELU:
        return torch.relu(s)
    if act == ext.ACT_GELU:
        return torch.nn.functional.gelu(s)
    return torch.nn.functional.silu(s)


def _dact64(act, s):
    s = s.detach().clone().requires_grad_(True)
    g, = torch.autograd.grad(_act64(act, s).sum(), s)
    return g


SIZES = [70, 0, 200, 33]


def _bf(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(BF)


# ------------------------------------------------------------------ the GEMM with the K extension

def _ext_case(orient, r, shared, gathered, seed=0):
    """orient 'fwd': W_g(n, k) k-contiguous (x W1_g^T); 'dx': n-contiguous (ds W1_g, w_ldn = 1)"""
    gen = torch.Generator().manual_seed(seed)
    G, P, T = len(SIZES), sum(SIZES), 150
    offsets = torch.tensor([0] + torch.tensor(SIZES).cumsum(0).tolist(), dtype=torch.int32)
    if orient == 'fwd':
        n, k = 192, 128
        w = _bf([G * n, k], gen)
        view = (n, k, n * k, k, 1)
    else:
        n, k = 128, 64                                 # W_g(n, kk) = w[g * k + kk, n]: d x bs blocks
        w = _bf([G * k, n], gen)
        view = (n, k, k * n, 1, n)
    a_rows = T if gathered else P
    a = _bf([a_rows, k], gen)
    gather = torch.randint(0, T, [P], generator=gen, dtype=torch.int32) if gathered else None
    a2 = torch.randn([a_rows, r], generator=gen)
    gather2 = gather
    b2 = _bf([n, r] if shared else [G * n, r], gen)
    return dict(G=G, P=P, n=n, k=k, w=w, view=view, a=a, gather=gather, a2=a2, gather2=gather2, b2=b2,
                b2gs=0 if shared else n * r, offsets=offsets,
                rowscale=torch.rand([P], generator=gen) + 0.5, bias=_bf([G, n], gen))


def _ext_ref(c, bias, rowscale):
    """fp64: rowscale (a W_g^T + bias) + a2 b2_g^T on the widened values"""
    n, k, gs, ldn, ldk = c['view']
    flat = c['w'].double().reshape(-1)
    out = torch.zeros([c['P'], n], dtype=torch.float64)
    offs = c['offsets'].tolist()
    for g in range(c['G']):
        lo, hi = offs[g], offs[g + 1]
        if hi == lo:
            continue
        wg = torch.as_strided(flat, (n, k), (ldn, ldk), g * gs)
        src = c['gather'][lo:hi].long() if c['gather'] is not None else torch.arange(lo, hi)
        v = c['a'].double()[src] @ wg.T
        if bias is not None:
            v = v + bias.double()[g]
        if rowscale is not None:
            v = v * rowscale.double()[lo:hi, None]
        b2 = c['b2'].double().reshape(-1)[g * c['b2gs']:g * c['b2gs'] + n * c['a2'].size(1)].view(n, -1)
        out[lo:hi] = v + c['a2'].double()[src] @ b2.T
    return out


def _run_ext(c, **kw):
    from naive_gpt import ext
    n, k, gs, ldn, ldk = c['view']
    cu = lambda t: t.cuda() if t is not None else None
    return ext.grouped_gemm_bf16_ext(
        cu(c['a']), cu(c['w']), cu(c['offsets']), c['G'], n=n, k=k, w_group_stride=gs, w_ldn=ldn, w_ldk=ldk,
        n_rows=c['P'], gather=cu(c['gather']), a2=cu(c['a2']), gather2=cu(c['gather2']), b2=cu(c['b2']),
        b2_group_stride=c['b2gs'], **{key: cu(v) if isinstance(v, torch.Tensor) else v for key, v in kw.items()})


@pytest.mark.parametrize('orient', ['fwd', 'dx'])
@pytest.mark.parametrize('r', [4, 16, 32])
@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('gathered', [False, True])
def test_ext_plain_against_fp64(orient, r, shared, gathered):
    c = _ext_case(orient, r, shared, gathered, seed=r)
    bias = c['bias'] if orient == 'fwd' else None
    got = _run_ext(c, bias=bias, rowscale=c['rowscale'])
    assert got.dtype == BF
    assert _bar(got, _ext_ref(c, bias, c['rowscale']))
    # accumulate: out = bf16(out + product)
    base = torch.randn(got.shape).to(BF)
    acc = _run_ext(c, rowscale=c['rowscale'], out=base.cuda().clone(), accumulate=True)
    assert _bar(acc, base.double() + _ext_ref(c, None, c['rowscale']))


@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('r', [4, 16, 32])
def test_ext_activation_against_fp64(act, r):
    from naive_gpt import ext
    c = _ext_case('fwd', r, False, True, seed=10 + r)
    h, pre = _run_ext(c, bias=c['bias'], rowscale=c['rowscale'], epilogue=ext.EPI_ACT, activation=act,
                      keep_preact=True)
    want = _ext_ref(c, c['bias'], c['rowscale'])
    assert _bar(pre, want) and _bar(h, _act64(act, want))


@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('orient', ['fwd', 'dx'])
def test_ext_dact_with_dots_against_fp64(act, orient):
    from naive_gpt import ext
    c = _ext_case(orient, 16, orient == 'dx', True, seed=20 + act)
    gen = torch.Generator().manual_seed(act)
    s = _bf([c['P'], c['n']], gen)
    h = _act64(act, s.double()).to(BF)
    kw = dict(h_in=h) if act == ext.ACT_RELU else dict(s_in=s)
    out, dot_main, dot_act = _run_ext(c, rowscale=c['rowscale'], epilogue=ext.EPI_DACT, activation=act,
                                      want_dots=True, **kw)
    v = _ext_ref(c, None, c['rowscale'])
    sv = h.double() if act == ext.ACT_RELU else s.double()
    hv = h.double() if act == ext.ACT_RELU else _act64(act, s.double())
    want = v * (sv > 0 if act == ext.ACT_RELU else _dact64(act, sv))
    assert _bar(out, want)
    assert _bar(dot_main.double().sum(1), (v * hv).sum(1))
    assert _bar(dot_act.double().sum(1), (want * sv).sum(1))


def test_ext_refuses_unsupported_ranks_and_mixes():
    c = _ext_case('fwd', 16, False, False)
    with pytest.raises(RuntimeError):
        _run_ext(dict(c, a2=torch.randn([c['P'], 36]), b2=_bf([c['G'] * c['n'], 36], torch.Generator())))
    with pytest.raises(RuntimeError):
        _run_ext(dict(c, a2=c['a2'].to(BF)))
    with pytest.raises(RuntimeError):
        _run_ext(dict(c, b2=c['b2'].float()))


# ------------------------------------------------------------------ lora_down, tall_tn, swiglu dots

@pytest.mark.parametrize('n', [4, 8, 16, 32, 48, 64])
def test_lora_down_bf16_against_fp64(n):
    from naive_gpt import ext
    gen = torch.Generator().manual_seed(n)
    x, l = _bf([300, 256], gen), _bf([256, n], gen, 0.1)
    u = ext.lora_down_bf16(x.cuda(), l.cuda())
    assert u.dtype == torch.float32 and u.shape == (300, n)
    assert _bar(u, x.double() @ l.double())
    if n % 16 == 0:
        ub = ext.lora_down_bf16(x.cuda(), l.cuda(), block_major=True)
        assert torch.equal(ub.permute(1, 0, 2).reshape(300, n), u)
    # a strided x (a column slice of a wider matrix) and the grouped form
    wide = _bf([300, 384], gen)
    assert _bar(ext.lora_down_bf16(wide.cuda()[:, 64:320], l.cuda()), wide.double()[:, 64:320] @ l.double())
    tables = _bf([len(SIZES), 256, n], gen, 0.1)
    offsets = torch.tensor([0] + torch.tensor(SIZES).cumsum(0).tolist(), dtype=torch.int32)
    xg = _bf([sum(SIZES), 256], gen)
    ug = ext.lora_down_grouped_bf16(xg.cuda(), tables.cuda(), offsets.cuda())
    want = torch.cat([xg.double()[lo:hi] @ tables.double()[g]
                      for g, (lo, hi) in enumerate(zip(offsets[:-1].tolist(), offsets[1:].tolist()))])
    assert ug.dtype == torch.float32 and _bar(ug, want)


@pytest.mark.parametrize('n', [4, 8, 16, 32, 48])
@pytest.mark.parametrize('grouped', [False, True])
def test_tall_tn_bf16_against_fp64_and_reproducible(n, grouped):
    from naive_gpt import ext
    gen = torch.Generator().manual_seed(100 + n)
    P, T, W = sum(SIZES) * 3, 257, 192
    wide = _bf([P, W], gen)
    sizes = [3 * s for s in SIZES]
    if grouped:
        offsets = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32)
        gather = torch.randint(0, T, [P], generator=gen, dtype=torch.int32)
        narrow = torch.randn([T, n], generator=gen)
        rows = narrow[gather.long()].double()
        want = torch.stack([wide.double()[lo:hi].T @ rows[lo:hi]
                            for lo, hi in zip(offsets[:-1].tolist(), offsets[1:].tolist())])
        args = dict(gather=gather.cuda(), offsets=offsets.cuda())
    else:
        narrow = torch.randn([P, n], generator=gen)
        want = (wide.double().T @ narrow.double())[None]
        args = {}
    got = ext.tall_tn_bf16(wide.cuda(), narrow.cuda(), **args)
    again = ext.tall_tn_bf16(wide.cuda(), narrow.cuda(), **args)
    assert got.dtype == BF and got.shape == want.shape
    assert _bar(got, want) and _one_rounding(got, want)
    assert torch.equal(got, again)


def test_swiglu_dots_against_the_fp32_kernel():
    from naive_gpt import ext
    gen = torch.Generator().manual_seed(7)
    dh, g, s = (_bf([300, 512], gen) for _ in range(3))
    dg, ds, dot_h, dot_g, dot_s = ext.swiglu_backward_dots_bf16(dh.cuda(), g.cuda(), s.cuda())
    dg32, ds32, h32, g32, s32 = ext.swiglu_backward(dh.float().cuda(), g.float().cuda(), s.float().cuda())
    assert dg.dtype == ds.dtype == BF and dot_h.dtype == torch.float32
    assert _one_rounding(dg, dg32) and _one_rounding(ds, ds32)
    # the same rounded gradients as spt_swiglu_backward_bf16
    dg16, ds16 = ext.swiglu_backward_bf16(dh.cuda(), g.cuda(), s.cuda())
    assert torch.equal(dg, dg16) and torch.equal(ds, ds16)
    # the dots are those of the STORED values (fp64 on them: the kernel bar); the fp32 kernel's are those
    # of the unrounded ones, an element's rounding (2^-9) apart: the layer bar
    h = (torch.nn.functional.silu(g.double()) * s.double()).to(BF).double()
    assert _bar(dot_h, (dh.double() * h).sum(1)) and _layer_close(dot_h, h32)
    assert _bar(dot_g, (dg.double().cpu() * g.double()).sum(1)) and _layer_close(dot_g, g32)
    assert _bar(dot_s, (ds.double().cpu() * s.double()).sum(1)) and _layer_close(dot_s, s32)


# ------------------------------------------------------------------ the layers

def _lora_layer(kind, d, dff, bs, r, act=None, seed=0):
    from naive_gpt import layers
    torch.manual_seed(seed)
    if kind == 'opt':
        m = layers.LoRARoutedFFN(d_lora=r, block_size=bs, d_model=d, d_feedforward=dff,
                                 activation=act or nn.ReLU())
    else:
        m = layers.LoRARoutedLLaMaFFN(d_lora=r, block_size=bs, d_model=d, d_feedforward=dff,
                                      activation=act or nn.SiLU())
    with torch.no_grad():
        for name, p in m.named_parameters():
            if 'lora' in name:
                p.copy_(torch.randn_like(p) * (0.05 if 'left' in name else 0.5))
            p.requires_grad_('lora' in name or 'router' in name)
    return m.cuda().to(BF)


def _trained(m):
    return [(n, p) for n, p in m.named_parameters() if p.requires_grad]


def _clear_tokens(m, n_tokens, d, seed):
    """inputs whose top-k blocks are the same in fp64 and in bf16, by a clear margin"""
    k = m.n_blocks // 2
    gen = torch.Generator().manual_seed(seed)
    pool = torch.randn([4 * n_tokens, d], generator=gen).cuda().to(BF)
    with torch.no_grad():
        p16 = m.router(pool).float()
        m64 = copy.deepcopy(m.router).double()
        p64 = m64(pool.double())
    top = torch.sort(p64, dim=-1, descending=True).values
    same = (torch.topk(p16, k, dim=-1).indices.sort(-1).values == torch.topk(p64, k, dim=-1).indices.sort(-1).values).all(-1)
    x = pool[same & (top[:, k - 1] - top[:, k] > 1e-2)][:n_tokens]
    assert x.size(0) == n_tokens
    return x.contiguous()


def _run(m, x, w):
    from naive_gpt import ext
    for _, p in _trained(m):
        p.grad = None
    x = x.detach().clone().requires_grad_(True)
    ext.reset_paths()
    y = m(x)
    (y * w).sum().backward()
    return y.detach(), x.grad, {n: p.grad for n, p in _trained(m)}, ext.paths_taken('routed_ffn')


class _AtBf16Router(nn.Module):
    """the fp64 router whose VALUES are those of the bf16 module's router (its bf16 Linear + Sigmoid is part
    of the layer: c = 2 prob carries its 2^-9, and next to a ReLU's kink that decides the mask) and whose
    derivative is the fp64 router's"""

    def __init__(self, router64, router16):
        super().__init__()
        self.router64, self.router16 = router64, router16

    def forward(self, x):
        p = self.router64(x)
        with torch.no_grad():
            p16 = self.router16(x.to(BF)).double()
        return p + (p16 - p).detach()


def _fp64(m, x, w):
    """the lora_ffn.py formula in fp64 on the widened values (the module's own loop, in fp64), at the bf16
    router's probabilities"""
    m64 = copy.deepcopy(m).double()
    router64 = m64.router
    m64.router = _AtBf16Router(router64, m.router)
    y, gx, grads, _ = _run(m64, x.double(), w.double())
    grads = {n.replace('router.router64.', 'router.'): g for n, g in grads.items()}
    return y, gx, grads


SHAPES = {'small': (128, 512, 128, 16, 256), 'configs2': (1024, 4096, 1024, 16, 512)}


@pytest.mark.parametrize('kind,act', [('opt', 'relu'), ('opt', 'gelu'), ('llama', 'silu')])
@pytest.mark.parametrize('shape', ['small', 'configs2'])
def test_layers_take_the_fused_bf16_path(kind, act, shape, monkeypatch):
    from naive_gpt.layers.sparse import grouped
    d, dff, bs, r, T = SHAPES[shape]
    acts = {'relu': nn.ReLU(), 'gelu': nn.GELU(), 'silu': nn.SiLU()}
    m = _lora_layer(kind, d, dff, bs, r, act=acts[act], seed=1)
    x = _clear_tokens(m, T, d, seed=2)
    w = torch.randn([T, d], device='cuda').to(BF)
    monkeypatch.setattr(grouped, 'LORA_BF16', True)
    y, gx, grads, paths = _run(m, x, w)
    assert paths == {('routed_ffn', 'fused_bf16'): 1}
    assert y.dtype == BF and gx.dtype == BF and all(g.dtype == BF for g in grads.values())
    y64, gx64, grads64 = _fp64(m, x, w)
    assert _layer_close(y, y64) and _layer_close(gx, gx64)
    for name, g in grads.items():
        # the router's gradients are sums over the tokens of coefficient gradients, each a difference of
        # row dots of bf16 tensors divided by c: the worst-conditioned outputs of the layer (the bf16 loop
        # misses fp64 by up to 8e-2 of scale on them at these shapes)
        assert _layer_close(g, grads64[name], 5e-2 if name.startswith('router') else 1e-2), name
    # against the bf16 per-block loop (flag off: the path of today).  Its ReLU mask is the sign of a
    # pre-activation rounded to bf16 several times (0.1 - 1 % of the elements differ from fp64's at these
    # shapes): behind a ReLU the two are compared on y only
    monkeypatch.setattr(grouped, 'LORA_BF16', False)
    yl, gxl, gradsl, paths_l = _run(m, x, w)
    assert paths_l == {('routed_ffn', 'torch_loop'): 1}
    assert _layer_close(y, yl, 2e-2)
    if act != 'relu':
        assert _layer_close(gx, gxl, 2e-2)
        for name, g in grads.items():
            # (the router's: both paths' errors of up to 5e-2 and 8e-2 of scale, see above)
            assert _layer_close(g, gradsl[name], 1e-1 if name.startswith('router') else 2e-2), name


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_exact_ties_go_to_the_lower_block(kind, monkeypatch):
    """tokens whose router probabilities tie exactly: the fused path keeps the lower block index"""
    from naive_gpt.layers.sparse import grouped
    d, dff, bs, r = 128, 512, 128, 16
    m = _lora_layer(kind, d, dff, bs, r, seed=3)
    with torch.no_grad():
        m.router[0].weight[3].copy_(m.router[0].weight[2])       # blocks 2 and 3 tie for every token
        m.router[0].bias[3].copy_(m.router[0].bias[2])
        m.router[0].weight[0].mul_(0.0).add_(m.router[0].weight[2])
        m.router[0].bias[0].copy_(m.router[0].bias[2] + 4.0)      # block 0 always first
        m.router[0].weight[1].mul_(0.0).add_(m.router[0].weight[2])
        m.router[0].bias[1].copy_(m.router[0].bias[2] - 4.0)      # block 1 always last
    x = torch.randn([64, d], device='cuda').to(BF)
    with torch.no_grad():
        prob = m.router(x).float()
    bk = grouped.make_buckets(prob, k=2, scale=2.0)
    # every token: blocks 0 and 2 (the lower of the tie)
    assert bk.offsets.tolist() == [0, 64, 64, 128, 128]
    monkeypatch.setattr(grouped, 'LORA_BF16', True)
    y, _, _, paths = _run(m, x, torch.ones_like(x))
    assert paths == {('routed_ffn', 'fused_bf16'): 1} and torch.isfinite(y.float()).all()


def _loop_opt(m, x):
    """LoRARoutedFFN's per-block loop, as lora_ffn.py writes it"""
    from naive_gpt.layers.sparse import routing
    prob = m.router(x)
    route = routing.route_topk(prob, k=m.n_blocks // 2)
    nb, bs = m.n_blocks, m.block_size
    b1 = m.fc1.bias.view([nb, bs])
    w1 = m.fc1.weight.view([nb, bs, -1])
    r1 = m.fc1.lora.right.weight.view([nb, bs, -1])
    l1 = m.fc1.lora.left.weight
    w2 = m.fc2.weight.view([-1, nb, bs])
    l2 = m.fc2.lora.left.weight.view([nb, bs, -1])
    r2 = m.fc2.lora.right.weight

    def block_fn(i, x_i, coeff):
        h = coeff * torch.addmm(b1[i], x_i, w1[i].T)
        h = h + torch.matmul(torch.matmul(x_i, l1), r1[i].T)
        h = m.activation(h)
        side = torch.matmul(torch.matmul(h, l2[i]), r2.T)
        return side + coeff * torch.matmul(h, w2[:, i, :].T)

    return routing.routed_apply(x, route, block_fn, weighted=True) + m.fc2.bias.view([1, -1])


def _loop_llama(m, x):
    from naive_gpt.layers.sparse import routing
    prob = m.router(x)
    route = routing.route_topk(prob, k=m.n_blocks // 2)
    nb, bs = m.n_blocks, m.block_size
    wg, rg, lg = m.gate.weight.view([nb, bs, -1]), m.gate.lora.right.weight.view([nb, bs, -1]), m.gate.lora.left.weight
    ws, rs, ls = m.side.weight.view([nb, bs, -1]), m.side.lora.right.weight.view([nb, bs, -1]), m.side.lora.left.weight
    wd, ld, rd = m.down.weight.view([-1, nb, bs]), m.down.lora.left.weight.view([nb, bs, -1]), m.down.lora.right.weight

    def block_fn(i, x_i, coeff):
        h_gate = coeff * torch.matmul(x_i, wg[i].T) + torch.matmul(torch.matmul(x_i, lg), rg[i].T)
        h_side = coeff * torch.matmul(x_i, ws[i].T) + torch.matmul(torch.matmul(x_i, ls), rs[i].T)
        h = m.activation(h_gate) * h_side
        return coeff * torch.matmul(h, wd[:, i, :].T) + torch.matmul(torch.matmul(h, ld[i]), rd.T)

    return routing.routed_apply(x, route, block_fn, weighted=True)


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_flag_off_is_the_loop_bitwise(kind, monkeypatch):
    from naive_gpt.layers.sparse import grouped
    d, dff, bs, r, T = 128, 512, 128, 16, 256
    m = _lora_layer(kind, d, dff, bs, r, seed=5)
    x = torch.randn([T, d], device='cuda').to(BF)
    w = torch.randn([T, d], device='cuda').to(BF)
    monkeypatch.setattr(grouped, 'LORA_BF16', False)
    y, gx, grads, paths = _run(m, x, w)
    assert paths == {('routed_ffn', 'torch_loop'): 1}
    for _, p in _trained(m):
        p.grad = None
    xr = x.clone().requires_grad_(True)
    yr = (_loop_opt if kind == 'opt' else _loop_llama)(m, xr)
    (yr * w).sum().backward()
    assert torch.equal(y, yr.detach()) and torch.equal(gx, xr.grad)
    for name, p in _trained(m):
        assert torch.equal(grads[name], p.grad), name


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_two_adamw_steps_train_the_tables_and_router(kind, monkeypatch):
    from naive_gpt.layers.sparse import grouped
    d, dff, bs, r, T = 128, 512, 128, 16, 256
    m = _lora_layer(kind, d, dff, bs, r, seed=6)
    x = torch.randn([T, d], device='cuda').to(BF)
    target = torch.randn([T, d], device='cuda').to(BF)
    monkeypatch.setattr(grouped, 'LORA_BF16', True)
    params = [p for _, p in _trained(m)]
    before = [p.detach().clone() for p in params]
    opt = torch.optim.AdamW(params, lr=1e-2)
    for _ in range(2):
        opt.zero_grad()
        loss = (m(x).float() - target.float()).square().mean()
        loss.backward()
        assert torch.isfinite(loss)
        opt.step()
    for (name, p), p0 in zip(_trained(m), before):
        assert not torch.equal(p, p0), name
        assert torch.isfinite(p.float()).all(), name


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_graph_capture_replays_bitwise(kind, monkeypatch):
    from naive_gpt.layers.sparse import grouped
    d, dff, bs, r, T = 256, 1024, 128, 16, 512
    m = _lora_layer(kind, d, dff, bs, r, seed=7)
    monkeypatch.setattr(grouped, 'LORA_BF16', True)
    x = torch.randn([T, d], device='cuda').to(BF).requires_grad_(True)
    w = torch.randn([T, d], device='cuda').to(BF)
    params = [p for _, p in _trained(m)]

    def step():
        x.grad = None
        for p in params:
            p.grad = None
        y = m(x)
        (y * w).sum().backward()
        return y

    y_eager = step().detach().clone()
    grads_eager = [x.grad.clone()] + [p.grad.clone() for p in params]
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
def test_recompute_origin_is_handed_over(kind, monkeypatch):
    """a norm output tagged by tuning/recompute.py: the fused bf16 path keeps the origin and recomputes x in
    its backward, with the gradients of the untagged run"""
    from naive_gpt.layers.sparse import grouped
    from naive_gpt.layers.tuning import recompute
    d, dff, bs, r, T = 128, 512, 128, 16, 256
    m = _lora_layer(kind, d, dff, bs, r, seed=8)
    norm = nn.LayerNorm(d).cuda().to(BF)
    monkeypatch.setattr(grouped, 'LORA_BF16', True)
    src = torch.randn([T, d], device='cuda').to(BF)
    w = torch.randn([T, d], device='cuda').to(BF)
    from naive_gpt.layers.basic import fused_norm
    outs = []
    for tagged in (False, True):
        for p in m.parameters():
            p.grad = None
        s = src.clone().requires_grad_(True)
        _, h = fused_norm.add_norm(norm, s, None)
        if tagged:
            h = recompute.tag(h, norm, s)
            assert recompute.origin_of(h) is not None
        (m(h) * w).sum().backward()
        outs.append([s.grad] + [p.grad for _, p in _trained(m)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
