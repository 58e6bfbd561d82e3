"""The routed FFN's router in fewer launches, bit for bit against the launches it replaces:

* forward: spt_lora_down2_route leaves the per-group selection counts beside the router's logits, and
  spt_route_topk_counted sums them instead of ranking every token in every workgroup;
* backward: spt_ffn_router_backward is spt_ffn_coeff_grad + two spt_rows_combine + spt_route_logit_backward.

Comparisons are on BITS (poison.same_bits): what torch.equal asks, and NaNs (the planted NaN row's
probabilities) and the sign of zeros compare too.
"""
import pytest
import torch
from torch import nn

import guard
from poison import PATTERNS, poisoned, same_bits

pytestmark = pytest.mark.gpu

K, RANK = 32, 16                # the smallest contraction and the one adapter rank lora_down_supported admits
FLOOR = 1e-12
ROUTE_NAMES = ('prob', 'token', 'block', 'offsets', 'pos', 'token64', 'block64', 'coeff')


def _cuda(t):
    return t.cuda()


# ---- forward ---------------------------------------------------------------------------------------

def _router_inputs(T, G, seed, dev=_cuda):
    """x [T, K], L1 [K, 16], router weight [G, K] and bias [G]: seeded, plus (T >= 15) five planted rows whose
    logits are exact by construction -- columns 0 and 1 of the weight are a +-1 pattern and a pattern with its
    maximum twice, and a planted x row is a multiple of a unit vector."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn([T, K], generator=gen)
    l1 = torch.randn([K, RANK], generator=gen) * 0.1
    rw = torch.randn([G, K], generator=gen) * 0.2
    rw[:, 0] = torch.tensor([1.0, -1.0] * (G // 2))
    rw[:, 1] = torch.tensor([1.0, 0.5, 1.0, 0.25] * (G // 4))
    bias = torch.randn([G], generator=gen) * 0.01
    if T >= 15:
        x[1] = float('nan')                                   # every logit NaN
        x[5] = 0.0                                            # equal logits (0): the bias alone ranks, and
        x[7] = 0.0                                            # ... ties go to the lower block
        x[7, 0] = 40.0                                        # logits +-40: sigmoids that round to 1 and ~0
        x[9] = 0.0
        x[9, 1] = 3.0                                         # the maximum twice (blocks 0 and 2)
        x[T - 1] = 0.0
        x[T - 1, 0] = -40.0
    return dev(x), dev(l1), dev(rw), dev(bias)


def _histogram(token, block, T, G):
    from naive_gpt import ext
    width = ext.route_counts_width(G)
    groups = (T + 15) // 16
    return torch.bincount((token.long() // 16) * width + block.long(), minlength=groups * width).int().view(groups, width)


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('G', [4, 8])
@pytest.mark.parametrize('T', [1, 15, 16, 17, 255, 256, 257, 700])
def test_counts_equal_the_histogram_and_the_counted_routing_equals_the_uncounted(T, G, k):
    from naive_gpt import ext
    x, l1, rw, bias = _router_inputs(T, G, seed=100 * T + 10 * G + k)
    assert ext.lora_down_supported(x, l1)
    plain = ext.lora_down(x, l1, block_major=True, exact=True, table2=rw)
    pack, image, norms, counts = ext.lora_down(x, l1, block_major=True, exact=True, table2=rw, route=(bias, k))
    assert image is None and norms is None
    assert same_bits(pack, plain), 'u / the logits changed with the counting'
    logits = pack[1]
    if T >= 15:
        assert torch.isnan(logits[1, :G]).all() and (logits[5, :G] == 0).all()
        assert logits[7, :G].tolist() == [40.0, -40.0] * (G // 2) and logits[9, 0] == logits[9, 2] == 3.0
    old = ext.route_topk_logits(logits, bias, G, k, 2.0)
    assert counts.dtype == torch.int32 and counts.shape == ((T + 15) // 16, ext.route_counts_width(G))
    assert torch.equal(counts, _histogram(old[1], old[2], T, G))
    assert int(counts.sum()) == T * k
    new = ext.route_topk_logits(logits, bias, G, k, 2.0, counts=counts)
    for name, a, b in zip(ROUTE_NAMES, new, old):
        assert same_bits(a, b), name


def test_counts_beside_the_image_and_norms_and_without_bias():
    """The by-product forms of the launch (the headline's: image and norms) and a router without bias."""
    from naive_gpt import ext
    T, G, k = 300, 4, 2
    x, l1, rw, _ = _router_inputs(T, G, seed=5)
    x = torch.nan_to_num(x, nan=0.5)                          # (row norms and the image of a NaN row: not the point)
    for want_image, want_norms in ((True, True), (True, False), (False, True)):
        plain = ext.lora_down(x, l1, want_image=want_image, want_norms=want_norms, block_major=True, exact=True,
                              table2=rw)
        pack, image, norms, counts = ext.lora_down(x, l1, want_image=want_image, want_norms=want_norms,
                                                   block_major=True, exact=True, table2=rw, route=(None, k))
        assert same_bits(pack, plain[0])
        assert (image is None) == (not want_image) and (norms is None) == (not want_norms)
        if want_image:
            assert same_bits(image.buffer, plain[1].buffer)
        if want_norms:
            assert same_bits(norms, plain[2])
        old = ext.route_topk_logits(pack[1], None, G, k, 2.0)
        assert torch.equal(counts, _histogram(old[1], old[2], T, G))
        new = ext.route_topk_logits(pack[1], None, G, k, 2.0, counts=counts)
        for name, a, b in zip(ROUTE_NAMES, new, old):
            assert same_bits(a, b), name


# ---- backward --------------------------------------------------------------------------------------

def _backward_inputs(T, G, k, w, seed, dev=_cuda):
    """The operands of the four calls at rank 16, with -0.0 entries in du and z (whole rows of one token, and
    scattered ones) and coefficients below the floor (0 and 1e-20)."""
    from naive_gpt import ext
    gen = torch.Generator().manual_seed(seed)
    prob = dev(torch.rand([T, G], generator=gen))
    token, block, offsets, pos, _, _, coeff = ext.route_topk_coeff(prob, k, 2.0)
    P = T * k
    rnd = lambda *shape: torch.randn(list(shape), generator=gen)
    du, z = rnd(P, RANK), rnd(P, RANK)
    rows = pos[T // 2].cpu().long()                           # every row of one token: 0 + (-0) + (-0) = +0
    du[rows] = -0.0
    z[rows] = -0.0
    du.view(-1)[::37] = -0.0
    z.view(-1)[::41] = -0.0
    coeff = coeff.cpu().clone()
    coeff[::5] = 0.0
    coeff[1::7] = 1e-20
    return dict(dot_main=dev(rnd(P, w)), dot_act=dev(rnd(P, w)), du=dev(du), u=dev(rnd(T, RANK)),
                dzt=dev(rnd(T, RANK)), z=dev(z), token=token, coeff=dev(coeff), pos=pos, block=block,
                prob=dev(torch.sigmoid(rnd(T, G))))


def _four_calls(a, G):
    from naive_gpt import ext
    rows = ext.ffn_coeff_grad(a['dot_main'], a['dot_act'], a['du'], a['u'], a['dzt'], a['z'], a['token'],
                              a['coeff'], FLOOR)
    du_tok = ext.rows_combine(a['du'], a['pos'])
    z_tok = ext.rows_combine(a['z'], a['pos'])
    dlogit = ext.route_coeff_backward(rows, a['pos'], a['block'], 2.0, G, prob=a['prob'])
    return dlogit, du_tok, z_tok, rows


def _one_call(a, want_rows=True):
    from naive_gpt import ext
    return ext.ffn_coeff_grad(a['dot_main'], a['dot_act'], a['du'], a['u'], a['dzt'], a['z'], a['token'],
                              a['coeff'], FLOOR, router=(a['pos'], a['block'], a['prob'], 2.0),
                              want_rows=want_rows)


@pytest.mark.parametrize('w', [2, 16])
@pytest.mark.parametrize('G', [4, 8])
@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('T', [1, 255, 256, 257, 1000])
def test_one_backward_launch_equals_the_four_it_replaces(T, k, G, w):
    a = _backward_inputs(T, G, k, w, seed=1000 * T + 100 * k + 10 * G + w)
    want = _four_calls(a, G)
    got = _one_call(a)
    for name, x, y in zip(('dlogit', 'du_tok', 'z_tok', 'per-row gradient'), got, want):
        assert same_bits(x, y), name
    assert not torch.signbit(got[1][T // 2]).any() and (got[1][T // 2] == 0).all(), 'a sum of -0.0 rows is +0.0'
    assert torch.isfinite(got[3]).all() and got[3].abs().max() > 1e9, 'no coefficient below the floor was hit'
    lean = _one_call(a, want_rows=False)
    assert lean[3] is None and all(same_bits(x, y) for x, y in zip(lean[:3], want[:3]))


# ---- poisoned buffers and guard bands: one case per new launch ----------------------------------------

def _flat(outs):
    flat = []
    for o in outs if isinstance(outs, (tuple, list)) else [outs]:
        if isinstance(o, (tuple, list)):
            flat += _flat(o)
        elif isinstance(o, torch.Tensor):
            flat.append(o)
        elif o is not None:
            flat.append(o.buffer)                             # a SplitImage
    return flat


def _case_counts(dev):
    from naive_gpt import ext
    x, l1, rw, bias = _router_inputs(300, 4, seed=21, dev=dev)        # 300 rows: a last tile of 12
    return lambda: ext.lora_down(x, l1, want_image=True, want_norms=True, block_major=True, exact=True, table2=rw,
                                 route=(bias, 2))


def _case_counted(dev):
    from naive_gpt import ext
    x, l1, rw, bias = _router_inputs(300, 8, seed=22)
    pack, _, _, counts = ext.lora_down(x, l1, block_major=True, exact=True, table2=rw, route=(bias, 2))
    logits, counts, bias = dev(pack[1].cpu()), dev(counts.cpu()), dev(bias.cpu())
    return lambda: ext.route_topk_logits(logits, bias, 8, 2, 2.0, counts=counts)


def _case_backward(dev):
    a = _backward_inputs(301, 4, 2, 16, seed=23)
    a = {name: dev(t.cpu()) for name, t in a.items()}
    return lambda: _one_call(a)


LAUNCHES = [('lora_down2_route', _case_counts), ('route_topk_counted', _case_counted),
            ('ffn_router_backward', _case_backward)]


@pytest.mark.parametrize('name,build', LAUNCHES, ids=[n for n, _ in LAUNCHES])
def test_launch_writes_every_output_element(name, build):
    """Under each poison every output has the bits of the zero run: no element is left as allocated."""
    call = build(_cuda)
    runs = {}
    for pattern in PATTERNS:
        with poisoned(pattern) as state:
            outs = call()
            torch.cuda.synchronize()
        assert state.count > 0 and not state.unclassified
        runs[pattern] = [o.clone() for o in _flat(outs)]
    for pattern in PATTERNS[1:]:
        assert len(runs[pattern]) == len(runs['zero']) > 0
        for i, (a, b) in enumerate(zip(runs['zero'], runs[pattern])):
            assert same_bits(a, b), '{}: output {} under {} differs from the zero run'.format(name, i, pattern)


@pytest.mark.parametrize('name,build', LAUNCHES, ids=[n for n, _ in LAUNCHES])
def test_launch_stays_inside_its_buffers(name, build):
    """Operands and outputs between guard bands: no band changes, and the outputs have the bits of the
    plain run under both band patterns (nothing read outside an operand reaches a result)."""
    plain = [o.clone() for o in _flat(build(_cuda)())]
    torch.cuda.synchronize()
    for pattern in guard.PATTERNS:
        with guard.guarded(pattern) as state:
            call = build(lambda t: guard.home(t, state, caller=name))
            outs = call()
            torch.cuda.synchronize()
        outs = [o.clone() for o in _flat(outs)]
        state.verify()
        assert state.allocations > 0 and state.homes > 0 and state.unguarded == 0
        state.release()
        assert len(outs) == len(plain)
        for i, (a, b) in enumerate(zip(plain, outs)):
            assert same_bits(a, b), '{}: output {} under {} bands differs from the plain run'.format(name, i, pattern)


# ---- the layer --------------------------------------------------------------------------------------

def test_layer_takes_both_paths_and_equals_the_separate_launches(monkeypatch):
    """LoRARoutedFFN forward and backward at 2048 tokens, d 64, d_ff 256, 4 blocks: both new forms are noted as
    taken, and the output and every gradient have the bits of a second evaluation that runs the old calls."""
    from naive_gpt import ext, layers
    from naive_gpt.layers.sparse import grouped
    torch.manual_seed(11)
    d, dff, bs = 64, 256, 64
    m = layers.LoRARoutedFFN(d_lora=16, block_size=bs, d_model=d, d_feedforward=dff, activation=nn.ReLU()).cuda()
    for name, p in m.named_parameters():
        if name.endswith('lora.right.weight'):
            p.data.normal_(0, 0.05)
    x0 = torch.randn([8, 256, d], device='cuda')
    w = torch.randn([8, 256, d], device='cuda')

    def run():
        x = x0.clone().requires_grad_(True)
        m.zero_grad()
        ext.reset_paths()
        y = m(x)
        (y * w).sum().backward()
        grads = {name: p.grad.clone() for name, p in m.named_parameters() if p.grad is not None}
        paths = {site: ext.paths_taken(site) for site in ('routed_ffn', 'router', 'router_counts', 'router_backward')}
        return y.detach().clone(), x.grad.clone(), grads, paths

    y1, dx1, g1, paths = run()
    assert paths['routed_ffn'] == {('routed_ffn', 'fused'): 1}
    assert paths['router'] == {('router', 'rides_lora_down'): 1}
    assert paths['router_counts'] == {('router_counts', 'ride_lora_down'): 1}
    assert paths['router_backward'] == {('router_backward', 'one_launch'): 1}
    monkeypatch.setattr(grouped, 'ROUTER_COUNTS', False)
    monkeypatch.setattr(grouped, 'ROUTER_BACKWARD_FUSED', False)
    y0, dx0, g0, paths = run()
    assert paths['router_counts'] == {('router_counts', 'recounted'): 1}
    assert paths['router_backward'] == {('router_backward', 'separate'): 1}
    assert same_bits(y1, y0) and same_bits(dx1, dx0)
    assert set(g1) == set(g0) and len(g1) >= 6 and any(n.startswith('router') for n in g1)
    for name in g1:
        assert same_bits(g1[name], g0[name]), name
