"""GPU tier: table gradients that read a norm's INPUT and form the norm's output on load
(spt_tall_tn_norm; ext.tall_tn / ext.tall_tn_batch with `norm`, `narrow2`), against the composition they
replace -- add_layernorm_forward, then tall_tn on its output -- bit for bit.

The claim is "same bits", so there is no tolerance anywhere: the transform is the forward kernel's own
expression (csrc/norm_apply.h), every accumulator keeps its chain of FMAs over the rows, and the chunk
sums are added in the same order.  Layer level: one upgraded block with the path on and forced off
(recompute.lazy -> None) gives equal gradients, and the norm forward is not launched in the backward
of the q / k / v projection and the routed FFN.
"""
import math

import pytest
import torch

import poison

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-5


def _ext():
    from naive_gpt import ext as E
    return E


def _case(rows, d, n, rms, seed):
    """s as tests/test_gpu_arith_contract.py::_inputs makes activations: gaussian, rows scaled 2^-12 .. 1"""
    gen = torch.Generator().manual_seed(seed)
    s = torch.randn([rows, d], generator=gen, dtype=torch.float64)
    s = (s * torch.pow(2.0, -torch.randint(0, 13, [rows, 1], generator=gen).double())).float()
    gamma = 1 + 0.2 * torch.randn([d], generator=gen)
    beta = None if rms else 0.1 * torch.randn([d], generator=gen)
    narrow = torch.randn([rows, n], generator=gen) / math.sqrt(rows)
    narrow2 = torch.randn([rows, 4], generator=gen)
    to = lambda t: None if t is None else t.to(DEV)
    return to(s), to(gamma), to(beta), to(narrow), to(narrow2)


def _norm_of(E, s, gamma, beta, rms):
    _, y, mean, rstd = E.add_layernorm_forward(s, None, gamma, beta, EPS, rms)
    return y, (None if rms else mean, rstd, gamma, beta)


@pytest.mark.parametrize('rms', [False, True], ids=['layernorm', 'rms'])
@pytest.mark.parametrize('d', [1024, 512])
@pytest.mark.parametrize('rows', [8192, 1500])
@pytest.mark.parametrize('n', [16, 48])
def test_norm_on_load_equals_the_product_on_the_norm_output(rms, d, rows, n):
    E = _ext()
    s, gamma, beta, narrow, _ = _case(rows, d, n, rms, seed=rows + d + n)
    y, norm = _norm_of(E, s, gamma, beta, rms)
    for kw in [{}, {'transposed': True}, {'split16': True}]:
        want = E.tall_tn(y, narrow, **kw)
        got = E.tall_tn(s, narrow, norm=norm, **kw)
        assert got.shape == want.shape and torch.equal(got, want), kw
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0


@pytest.mark.parametrize('rms', [False, True], ids=['layernorm', 'rms'])
@pytest.mark.parametrize('d', [1024, 512])
@pytest.mark.parametrize('rows', [8192, 1500])
def test_two_narrow_operands_equal_the_two_products(rms, d, rows):
    """16 + 4 columns from one pass: both outputs equal the separate calls, in both layouts of the
    second one, on a plain `wide` and on a norm's input."""
    E = _ext()
    s, gamma, beta, narrow, narrow2 = _case(rows, d, 16, rms, seed=rows + d)
    y, norm = _norm_of(E, s, gamma, beta, rms)
    want = E.tall_tn(y, narrow)
    for transposed2 in (False, True):
        want2 = E.tall_tn(y, narrow2, transposed=transposed2)
        for wide, nm in ((y, None), (s, norm)):
            got, got2 = E.tall_tn(wide, narrow, norm=nm, narrow2=narrow2, transposed2=transposed2)
            assert got.shape == want.shape and torch.equal(got, want), (transposed2, nm is None)
            assert got2.shape == want2.shape and torch.equal(got2, want2), (transposed2, nm is None)
    # the first output in the layouts of spt_tall_tn
    for kw in [{'transposed': True}, {'split16': True}]:
        got, got2 = E.tall_tn(s, narrow, norm=norm, narrow2=narrow2, transposed2=True, **kw)
        assert torch.equal(got, E.tall_tn(y, narrow, **kw)) and torch.equal(got2, E.tall_tn(y, narrow2, transposed=True))


@pytest.mark.parametrize('rms', [False, True], ids=['layernorm', 'rms'])
@pytest.mark.parametrize('d', [1024, 512])
@pytest.mark.parametrize('rows', [8192, 1500])
@pytest.mark.parametrize('two', [False, True], ids=['16', '16+4'])
def test_mixed_batch_equals_the_single_calls(rms, d, rows, two):
    """The routed FFN's pair: (s -> x, du [, dlogit]) and a plain (dy, z) in one pair of launches."""
    E = _ext()
    s, gamma, beta, narrow, narrow2 = _case(rows, d, 16, rms, seed=rows + d + 1)
    gen = torch.Generator().manual_seed(5)
    dy = torch.randn([rows, d], generator=gen).to(DEV)
    z = torch.randn([rows, 16], generator=gen).to(DEV)
    y, norm = _norm_of(E, s, gamma, beta, rms)
    outs = E.tall_tn_batch([s, dy], [narrow, z], norms=[norm, None], narrows2=[narrow2, None] if two else None,
                           transposed2=True)
    first = outs[0][0] if two else outs[0]
    assert torch.equal(first, E.tall_tn(y, narrow))
    assert torch.equal(outs[1], E.tall_tn(dy, z))
    if two:
        assert torch.equal(outs[0][1], E.tall_tn(y, narrow2, transposed=True))
    # two problems on one norm's input (the gated FFN's two `left` tables)
    outs = E.tall_tn_batch([s, s], [narrow, z], norms=[norm, norm], narrows2=[narrow2, None] if two else None)
    assert torch.equal(outs[0][0] if two else outs[0], E.tall_tn(y, narrow))
    assert torch.equal(outs[1], E.tall_tn(y, z))
    if two:
        assert torch.equal(outs[0][1], E.tall_tn(y, narrow2))
    # and the other way round: the plain problem first, the norm an RMS / LayerNorm of the second
    outs = E.tall_tn_batch([dy, s], [z, narrow], norms=[None, norm], narrows2=[None, narrow2] if two else None)
    assert torch.equal(outs[0], E.tall_tn(dy, z))
    assert torch.equal(outs[1][0] if two else outs[1], E.tall_tn(y, narrow))
    if two:
        assert torch.equal(outs[1][1], E.tall_tn(y, narrow2))


@pytest.mark.parametrize('rms', [False, True], ids=['layernorm', 'rms'])
@pytest.mark.parametrize('pattern', poison.PATTERNS)
def test_poisoned_outputs_and_workspace_change_nothing(rms, pattern):
    """Outputs and the chunk workspace filled before the call (tests/poison.py): same bits, no NaN --
    the unwritten second-operand rows of a problem without one are never read."""
    E = _ext()
    rows, d = 1500, 1024
    s, gamma, beta, narrow, narrow2 = _case(rows, d, 16, rms, seed=9)
    wide48 = torch.randn([rows, 48], generator=torch.Generator().manual_seed(2)).to(DEV)
    gen = torch.Generator().manual_seed(6)
    dy = torch.randn([rows, d], generator=gen).to(DEV)
    z = torch.randn([rows, 16], generator=gen).to(DEV)
    _, norm = _norm_of(E, s, gamma, beta, rms)

    def run():
        a = E.tall_tn(s, wide48, norm=norm, split16=True)
        b = E.tall_tn_batch([s, dy], [narrow, z], norms=[norm, None], narrows2=[narrow2, None], transposed2=True)
        return [a, b[0][0], b[0][1], b[1]]

    want = run()
    with poison.poisoned(pattern) as state:
        got = run()
    assert state.count >= 5 and not state.unclassified
    for g, w in zip(got, want):
        assert torch.isfinite(g).all() and poison.same_bits(g, w)


def test_arguments_are_checked_before_any_launch():
    E = _ext()
    s, gamma, beta, narrow, narrow2 = _case(1500, 1024, 16, False, seed=1)
    _, norm = _norm_of(E, s, gamma, beta, False)
    offsets = torch.tensor([0, 1500], dtype=torch.int32, device=DEV)
    with pytest.raises(Exception):
        E.tall_tn(s, narrow, norm=norm, offsets=offsets)                    # no groups in this mode
    with pytest.raises(Exception):
        E.tall_tn(s, narrow2, norm=norm)                                    # n = 4 alone
    with pytest.raises(Exception):
        E.tall_tn(s, narrow, norm=(norm[0], norm[1][:-1], gamma, beta))     # one rstd per row
    assert not E.tall_tn_norm_supported(s, narrow.repeat(1, 3), norm, narrow2)   # 48 + 4


# ------------------------------------------------------------------------------ layer level

BLOCKS = {
    # the headline's block (BERT-large dimensions, OPT wiring): LayerNorm, q / k / v and the routed FFN on load
    'opt': dict(family='opt', d=1024, heads=16, d_ff=4096, N=4, S=512, recomputed=0),
    # LLaMA wiring: RMS norms, q / k / v and the gated routed FFN (two `left` tables and the router) on load
    'llama': dict(family='llama', d=1024, heads=16, d_ff=4096, N=4, S=512, recomputed=0),
}


@pytest.mark.parametrize('name', list(BLOCKS))
def test_block_gradients_equal_with_the_path_on_and_off(name, monkeypatch):
    import test_gpu_fullsize_blocks as F
    from naive_gpt import ext
    from naive_gpt.layers.tuning import recompute
    c = BLOCKS[name]
    block = F._make_block(c)
    gen = torch.Generator().manual_seed(3)
    F._randomise_adapters(block, gen)
    x = torch.randn([c['N'], c['S'], c['d']], generator=gen).cuda()
    w = torch.randn([c['N'], c['S'], c['d']], generator=gen).cuda()
    calls = []
    forward = ext.add_layernorm_forward

    def counted(*args, **kwargs):
        calls.append(1)
        return forward(*args, **kwargs)

    def run():
        block.zero_grad()
        ext.drop_images()
        ext.reset_paths()
        xi = x.clone().requires_grad_(True)
        y = block(xi)
        loss = (y * w).sum()
        del calls[:]
        with monkeypatch.context() as m:
            m.setattr(ext, 'add_layernorm_forward', counted)
            loss.backward()
        grads = {n: p.grad.clone() for n, p in block.named_parameters() if p.grad is not None}
        return y.detach(), xi.grad, grads, len(calls), {k[1]: v for k, v in ext.paths_taken('norm_output').items()}

    y_on, gx_on, g_on, n_on, paths_on = run()
    with monkeypatch.context() as m:
        m.setattr(recompute, 'lazy', lambda origin: None)
        y_off, gx_off, g_off, n_off, paths_off = run()
    print('[norm on load] {}: norm forwards inside the backward {} -> {}, paths {} -> {}'.format(
        name, n_off, n_on, paths_off, paths_on))
    on_load = 2 - c['recomputed']                    # the consumers that note which way they took
    assert n_off == 2 and paths_off == {'recomputed': on_load}
    assert n_on == c['recomputed'] and paths_on == {'on_load': on_load}, (n_on, paths_on)
    assert torch.equal(y_on, y_off) and torch.equal(gx_on, gx_off)
    trainable = {n for n, p in block.named_parameters() if p.requires_grad}
    # (the PQ loss is not armed -- it reads no norm output -- so the quantizer's table has no gradient)
    assert set(g_on) == set(g_off) == trainable - {'mha.attn_fn.quantizer.weight'}
    assert any('lora.left' in n for n in g_on) and any('router' in n for n in g_on)
    for n in sorted(g_on):
        assert torch.equal(g_on[n], g_off[n]), n
