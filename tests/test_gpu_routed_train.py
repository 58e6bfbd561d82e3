"""GPU tier: training the plain routed FFNs on the grouped path (spt_grouped_gemm_wgrad).

The kernel against the fp64 per-group formula; RoutedFFN (ReLU) / RoutedLLaMaFFN (SiLU) with
grouped.TRAINABLE_WEIGHTS on against the imported reference's gradients (tests/golden/routed_train.npz),
at configs[2] FFN dims against the same layer in fp64 (which takes the loop), over two AdamW steps
against the loop, and captured in a HIP graph against eager."""
import os

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'routed_train.npz')


def _scaled_close(got, want, rtol=1e-3, frac=3e-4):
    """allclose with the absolute tolerance as a fraction of the reference's magnitude."""
    want = want.to(got.dtype)
    return torch.allclose(got, want, rtol=rtol, atol=frac * want.abs().max().item())


@pytest.fixture
def trainable(monkeypatch):
    from naive_gpt.layers.sparse import grouped
    monkeypatch.setattr(grouped, 'TRAINABLE_WEIGHTS', True)
    return grouped


# ------------------------------------------------------------------ the kernel

def ref_wgrad(grad, a, offsets, view, gather_g, gather_a, rowscale, size):
    n, k, gs, ldn, _ = view
    out = torch.zeros([size], dtype=torch.float64)
    dbias = torch.zeros([len(offsets) - 1, n], dtype=torch.float64)
    grad, a = grad.double().cpu(), a.double().cpu()
    for g in range(len(offsets) - 1):
        rows = torch.arange(offsets[g], offsets[g + 1])
        sg = gather_g.cpu().long()[rows] if gather_g is not None else rows
        sa = gather_a.cpu().long()[rows] if gather_a is not None else rows
        gr = grad[sg]
        if rowscale is not None:
            gr = gr * rowscale.double().cpu()[rows][:, None]
        idx = g * gs + torch.arange(n)[:, None] * ldn + torch.arange(k)[None, :]
        out[idx.reshape(-1)] = (gr.T @ a[sa]).reshape(-1)
        dbias[g] = gr.sum(0)
    return out, dbias


@pytest.mark.parametrize('gathers', ['none', 'g', 'a', 'both'])
@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('layout', ['fc1', 'fc2'])
def test_wgrad_matches_fp64_per_group_formula(gathers, scaled, layout):
    from naive_gpt import ext
    gen = torch.Generator().manual_seed(7)
    # ragged buckets: an empty one, a 1-row one, one longer than several chunks, a short one
    sizes = [37, 0, 1, 2113, 260]
    P, G = sum(sizes), len(sizes)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    if layout == 'fc1':     # W1 [G * n, k]: (n, k, n * k, k, 1); n, k not multiples of the tile
        n, k = 196, 100
        view, size = (n, k, n * k, k, 1), G * n * k
    else:                   # W2 [k_out, G * n_in] with n = d, k = block: (n, k, k, G * k, 1)
        n, k = 132, 64
        view, size = (n, k, k, G * k, 1), n * G * k
    T = 700
    grad = torch.randn([T if gathers in ('g', 'both') else P, n], generator=gen)
    a = torch.randn([T if gathers in ('a', 'both') else P, k], generator=gen)
    gather_g = torch.randint(0, T, [P], generator=gen, dtype=torch.int32) if gathers in ('g', 'both') else None
    gather_a = torch.randint(0, T, [P], generator=gen, dtype=torch.int32) if gathers in ('a', 'both') else None
    rowscale = torch.rand([P], generator=gen) + 0.5 if scaled else None
    want, want_bias = ref_wgrad(grad, a, offsets.tolist(), view, gather_g, gather_a, rowscale, size)

    def cuda(t):
        return t.cuda() if t is not None else None

    out = torch.full([size], float('nan'), device='cuda')                 # written whole
    got, dbias = ext.grouped_gemm_wgrad(cuda(grad), cuda(a), cuda(offsets), view, P, gather_grad=cuda(gather_g),
                                        gather_a=cuda(gather_a), rowscale=cuda(rowscale), out=out,
                                        want_bias=True)
    assert got is out and torch.isfinite(out).all() and torch.isfinite(dbias).all()
    scale = want.abs().max().item()
    assert (got.double().cpu() - want).abs().max().item() <= 1e-4 * scale
    assert torch.allclose(dbias.double().cpu(), want_bias, rtol=1e-5, atol=1e-4)
    assert (got.double().cpu()[want == 0] == 0).all()          # the empty group: zeros, no NaN left
    again, dbias2 = ext.grouped_gemm_wgrad(cuda(grad), cuda(a), cuda(offsets), view, P, gather_grad=cuda(gather_g),
                                           gather_a=cuda(gather_a), rowscale=cuda(rowscale), want_bias=True)
    assert torch.equal(again, got) and torch.equal(dbias2, dbias)       # bitwise reproducible


def test_grouped_linear_forms_weight_and_bias_gradients():
    """GroupedLinear.backward: the weight and bias gradients of out = s (a[gather] W_g^T + b_g) by the
    new call (it raised before), against the same product through torch autograd in fp64."""
    from naive_gpt.layers.sparse import grouped
    gen = torch.Generator().manual_seed(21)
    G, n, k, T = 4, 96, 64, 300
    sizes = [120, 0, 333, 47]
    P = sum(sizes)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32).cuda()
    a = torch.randn([T, k], generator=gen).cuda()
    gather = torch.randint(0, T, [P], generator=gen, dtype=torch.int32).cuda()
    weight = torch.randn([G * n, k], generator=gen).cuda().requires_grad_(True)
    bias = torch.randn([G, n], generator=gen).cuda().requires_grad_(True)
    scale = (torch.rand([P], generator=gen) + 0.5).cuda()
    dout = torch.randn([P, n], generator=gen).cuda()
    out = grouped.grouped_linear(a, weight, offsets, (n, k, n * k, k, 1), gather=gather,
                                 gather_long=gather.long(), bias=bias, rowscale=scale)
    out.backward(dout)
    w64 = weight.detach().double().requires_grad_(True)
    b64 = bias.detach().double().requires_grad_(True)
    block = torch.repeat_interleave(torch.arange(G, device='cuda'), torch.tensor(sizes, device='cuda'))
    w_rows = w64.view(G, n, k)[block]                                    # [P, n, k]
    ref = scale.double()[:, None] * (torch.einsum('pk,pnk->pn', a.double()[gather.long()], w_rows) + b64[block])
    ref.backward(dout.double())
    assert _scaled_close(out.detach(), ref.detach())
    assert _scaled_close(weight.grad, w64.grad)
    assert _scaled_close(bias.grad, b64.grad)
    assert (bias.grad[1] == 0).all()                                     # the empty group


def test_wgrad_rejects_bad_arguments_before_launch():
    from naive_gpt import ext
    lib = ext.load_library()
    x = torch.zeros([64, 64], device='cuda')
    off = torch.zeros([3], dtype=torch.int32, device='cuda')
    work = torch.empty([lib.spt_grouped_gemm_wgrad_workspace_bytes(64, 2, 64, 64)], dtype=torch.uint8,
                       device='cuda')
    p = x.data_ptr()
    assert lib.spt_grouped_gemm_wgrad(p, 64, None, p, 64, None, None, off.data_ptr(), 2, 64, 62, 64, p,
                                      64 * 64, 64, None, work.data_ptr(), None) == -2        # n % 4
    assert lib.spt_grouped_gemm_wgrad(p, 64, None, p, 64, None, None, off.data_ptr(), 2, 64, 64, 64, p,
                                      64 * 64, 32, None, work.data_ptr(), None) == -1        # ldn < k


# ------------------------------------------------------------------ the layers

def _golden_module(kind):
    from naive_gpt import layers
    z = np.load(GOLDEN)
    if kind == 'opt':
        m = layers.RoutedFFN(d_model=32, d_feedforward=512, block_size=64, activation=nn.ReLU())
    else:
        m = layers.RoutedLLaMaFFN(d_model=32, d_feedforward=512, block_size=64, activation=nn.SiLU())
    state = {key[len(kind) + 7:]: torch.from_numpy(z[key].astype(np.float32))
             for key in z.files if key.startswith(kind + '.param.')}
    m.load_state_dict(state)
    return m.cuda(), z


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_trainable_layers_match_the_reference_golden(kind, trainable):
    from naive_gpt import ext
    m, z = _golden_module(kind)
    x = torch.from_numpy(z[kind + '.x'].astype(np.float32)).cuda().requires_grad_(True)
    w = torch.from_numpy(z[kind + '.w'].astype(np.float32)).cuda()
    ext.reset_paths()
    y = m(x)
    (y * w).sum().backward()
    assert ext.paths_taken('routed_ffn_plain') == {('routed_ffn_plain', 'grouped_trainable'): 1}
    assert ext.paths_taken('route_topk') == {('route_topk', 'kernel'): 1}
    assert _scaled_close(y.cpu(), torch.from_numpy(z[kind + '.y']))
    assert _scaled_close(x.grad.cpu(), torch.from_numpy(z[kind + '.grad_x']))
    for name, p in m.named_parameters():
        if name.startswith('router'):
            assert bool(z[kind + '.router_grad_is_none.' + name]) and p.grad is None, name
        else:
            assert _scaled_close(p.grad.cpu(), torch.from_numpy(z[kind + '.grad.' + name])), name


def _separated_tokens(m, k, n_tokens, d, seed):
    """n_tokens inputs whose top-k router margin exceeds 1e-4 in fp64 (fp32 routing agrees)"""
    gen = torch.Generator().manual_seed(seed)
    pool = torch.randn([n_tokens + n_tokens // 4, d], generator=gen).cuda()
    with torch.no_grad():
        prob = m.router.double()(pool.double())
        m.router.float()
        top = torch.sort(prob, dim=-1, descending=True).values
        keep = (top[:, k - 1] - top[:, k]) > 1e-4
    x = pool[keep][:n_tokens]
    assert x.size(0) == n_tokens
    return x


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_configs2_ffn_dims_against_fp64(kind, trainable):
    """d 1024, d_ff 4096, block 1024, 4096 tokens: every gradient within 1e-3 of scale of the fp64
    layer (an inexact ReLU mask puts O(1) errors in rows of dW1)."""
    import copy
    from naive_gpt import ext, layers
    torch.manual_seed(3)
    d, dff, bs, T = 1024, 4096, 1024, 4096
    if kind == 'opt':
        m = layers.RoutedFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=nn.ReLU()).cuda()
        k = m.n_blocks // 2
    else:
        m = layers.RoutedLLaMaFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=nn.SiLU()).cuda()
        k = m.n_blocks // 4
    x = _separated_tokens(m, k, T, d, 5).requires_grad_(True)
    w = torch.randn([T, d], device='cuda')
    ext.reset_paths()
    y = m(x)
    (y * w).sum().backward()
    assert ext.paths_taken('routed_ffn_plain') == {('routed_ffn_plain', 'grouped_trainable'): 1}
    m64 = copy.deepcopy(m).double()
    x64 = x.detach().double().requires_grad_(True)
    y64 = m64(x64)
    (y64 * w.double()).sum().backward()
    assert _scaled_close(y, y64)
    assert _scaled_close(x.grad, x64.grad)
    for (name, p), p64 in zip(m.named_parameters(), m64.parameters()):
        if name.startswith('router'):
            assert p.grad is None and p64.grad is None
        else:
            assert _scaled_close(p.grad, p64.grad), name


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_two_adamw_steps_equal_the_loop(kind, trainable, monkeypatch):
    """Weight images and norms follow the weights across optimizer steps: after two AdamW steps on the
    grouped path, its output and gradients equal the loop's on the SAME weights (a stale image or norm
    would still describe the weights of an earlier step: an lr-sized error), and the weights equal two
    steps taken on the loop (to Adam's amplification of the split's 2^-16: tolerance 1e-2 of scale,
    against a 15 % change per step).  The two trajectories are compared by their updates as a whole:
    element by element they may part where a pre-activation near a ReLU's kink lands on different
    sides after the first step."""
    import copy
    from naive_gpt import ext, layers
    torch.manual_seed(9)
    d, dff, bs, T = 256, 1024, 128, 1024
    if kind == 'opt':
        m = layers.RoutedFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=nn.ReLU()).cuda()
        k = m.n_blocks // 2
    else:
        m = layers.RoutedLLaMaFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=nn.SiLU()).cuda()
        k = m.n_blocks // 4
    x = _separated_tokens(m, k, T, d, 1)
    w = torch.randn([T, d], device='cuda')
    ref = copy.deepcopy(m)
    start = [p.detach().clone() for p in m.parameters()]

    def loss_and_grads(model):
        model.zero_grad(set_to_none=True)
        y = model(x)
        (y * w).sum().backward()
        return y.detach().clone(), [p.grad.clone() if p.grad is not None else None for p in model.parameters()]

    for model, on in ((m, True), (ref, False)):
        monkeypatch.setattr(trainable, 'TRAINABLE_WEIGHTS', on)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-2, eps=1e-3)
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            (model(x) * w).sum().backward()
            opt.step()
    for (name, p), p_loop, p0 in zip(m.named_parameters(), ref.parameters(), start):
        step = (p_loop - p0).norm().item()
        assert (p - p_loop).norm().item() <= 0.05 * step, name     # (the router: no step, both equal)
    monkeypatch.setattr(trainable, 'TRAINABLE_WEIGHTS', True)
    ext.reset_paths()
    y, grads = loss_and_grads(m)
    assert ext.paths_taken('routed_ffn_plain') == {('routed_ffn_plain', 'grouped_trainable'): 1}
    monkeypatch.setattr(trainable, 'TRAINABLE_WEIGHTS', False)
    y_loop, grads_loop = loss_and_grads(m)
    assert _scaled_close(y, y_loop)
    for (name, _), g, g0 in zip(m.named_parameters(), grads, grads_loop):
        assert (g is None) == (g0 is None), name
        if g is not None:
            assert _scaled_close(g, g0), name


def _graph_capture_of_forward_and_backward(kind):
    from naive_gpt import layers
    torch.manual_seed(13)
    d, dff, bs, T = 256, 1024, 128, 512
    if kind == 'opt':
        m = layers.RoutedFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=nn.ReLU()).cuda()
    else:
        m = layers.RoutedLLaMaFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=nn.SiLU()).cuda()
    x = torch.randn([T, d], device='cuda', requires_grad=True)
    w = torch.randn([T, d], device='cuda')
    params = [p for p in m.parameters()]

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
    assert torch.allclose(y_static, y_eager, rtol=1e-6, atol=1e-7 * y_eager.abs().max().item())
    grads = [x.grad] + [p.grad for p in params]
    for g, ge in zip(grads, grads_eager):
        assert (g is None) == (ge is None)
        if g is not None:
            assert torch.allclose(g, ge, rtol=1e-6, atol=1e-7 * ge.abs().max().item())
    # The same graph on new contents of its buffers: new tokens, a new upstream gradient, and every
    # trained parameter nudged in place, as the in-graph optimiser moves it between two replays.
    # Whatever the capture took from a cache that the warm-up filled (row norms, kept images of the
    # weights) must follow: the replay equals an eager step on the new contents.
    with torch.no_grad():
        x.copy_(torch.randn_like(x))
        w.copy_(torch.randn_like(w))
        for p in params:
            if p.requires_grad:
                p.add_(0.01 * torch.randn_like(p))
    graph.replay()
    torch.cuda.synchronize()
    y_replay = y_static.detach().clone()
    grads_replay = [None if g is None else g.clone() for g in [x.grad] + [p.grad for p in params]]
    y_new = step().detach().clone()
    grads_new = [x.grad] + [p.grad for p in params]
    assert not torch.equal(y_new, y_eager), 'the new contents changed nothing'
    assert torch.allclose(y_replay, y_new, rtol=1e-6, atol=1e-7 * y_new.abs().max().item())
    for i, (g, ge) in enumerate(zip(grads_replay, grads_new)):
        assert (g is None) == (ge is None)
        if g is not None:
            assert torch.allclose(g, ge, rtol=1e-6, atol=1e-7 * ge.abs().max().item()), 'gradient %d' % i


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_graph_capture_of_forward_and_backward(kind, trainable):
    _graph_capture_of_forward_and_backward(kind)


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_graph_capture_with_kept_weight_images(kind, trainable, monkeypatch):
    """SPT_WEIGHT_IMAGES=keep: images and row norms of weights are kept with the parameter.  The
    trained weights' must follow the nudged weights all the same: the trainable path forms them
    from the weights' values at the call, and a capture is never served what eager code kept for a
    weight that requires a gradient (ext._PerParameter)."""
    from naive_gpt import ext
    monkeypatch.setattr(ext, 'KEEP_WEIGHT_IMAGES', True)
    ext.drop_images()
    try:
        _graph_capture_of_forward_and_backward(kind)
    finally:
        ext.drop_images()
