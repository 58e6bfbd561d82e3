"""GPU tier: the fused add + norm kernels at d_model 768 (a wave per row, three float4 per lane) and at
2560, 4096 (LayerNorm) and 5120 (the wide-row form of csrc/layernorm.hip: several waves share a row,
the row sums cross them through LDS in a fixed order).

Arbiter: fp64 -- nn.functional.layer_norm and the RMS formula of layers/basic/utils.py on .double()
inputs -- under the bound of tests/test_gpu_layernorm.py (rtol 1e-4, atol 1e-5 max|want|).  The fp32
library path (the op-by-op expression the parent of this change ran at these widths) is held to the same
bound on the same inputs, so a failure of the kernels cannot be blamed on the inputs.  At 4096 RMS is
the kernel that was there before: a control.
"""
import logging
import math

import pytest
import torch
from torch import nn

import poison

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-5
WIDTHS = (768, 2560, 4096, 5120)
NAMES = ('s', 'y', 'grad_x', 'grad_r', 'grad_gamma', 'grad_beta')


def _ext():
    from naive_gpt import ext as E
    return E


def _norm(d, rms, gen):
    """A norm module with the parameters of tests/test_gpu_layernorm.py: gamma 1 + 0.1 randn, beta 0.1 randn"""
    from naive_gpt import layers
    norm = (layers.LlamaRMSNorm(d, eps=EPS) if rms else nn.LayerNorm(d, eps=EPS)).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.1 * torch.randn([d], generator=gen))
        if not rms:
            norm.bias.copy_(0.1 * torch.randn([d], generator=gen))
    return norm


def _inputs(rows, d, add, gen):
    """x = 2 randn + 0.5, r and the two output weights randn, as tests/test_gpu_layernorm.py"""
    x = (2.0 * torch.randn([rows, d], generator=gen) + 0.5).to(DEV)
    r = torch.randn([rows, d], generator=gen).to(DEV) if add else None
    ws, wy = [torch.randn([rows, d], generator=gen).to(DEV) for _ in range(2)]
    return x, r, ws, wy


def _fp64(norm, rms, x, r, ws, wy):
    d = x.size(-1)
    xi = x.double().requires_grad_(True)
    ri = r.double().requires_grad_(True) if r is not None else None
    g = norm.weight.detach().double().requires_grad_(True)
    b = None if rms else norm.bias.detach().double().requires_grad_(True)
    s = xi + ri if r is not None else xi
    if rms:
        y = g * (s * torch.rsqrt(s.square().mean(dim=-1, keepdim=True) + EPS))
    else:
        y = nn.functional.layer_norm(s, [d], g, b, EPS)
    ((s * ws.double()).sum() + (y * wy.double()).sum()).backward()
    return (s.detach(), y.detach(), xi.grad, ri.grad if r is not None else None, g.grad, None if rms else b.grad)


def _fp32(norm, rms, x, r, ws, wy, fused):
    from naive_gpt.layers.basic import fused_norm
    xi = x.clone().requires_grad_(True)
    ri = r.clone().requires_grad_(True) if r is not None else None
    norm.zero_grad()
    if fused:
        assert fused_norm.usable(norm, xi)
        s, y = fused_norm.add_norm(norm, xi, ri)
    else:
        s = xi + ri if r is not None else xi
        y = norm(s)
    ((s * ws).sum() + (y * wy).sum()).backward()
    return (s.detach(), y.detach(), xi.grad, ri.grad if r is not None else None, norm.weight.grad.clone(),
            None if rms else norm.bias.grad.clone())


def _within(got, want, what):
    """The bound of tests/test_gpu_layernorm.py against the fp64 result; prints each figure first"""
    for a, b, name in zip(got, want, NAMES):
        if b is None:
            continue
        a = a.double()
        scale = b.abs().max().item()
        # the worst element's need of the absolute term, as a share of it (<= 0: rtol alone covers every element)
        need = ((a - b).abs() - 1e-4 * b.abs()).max().item() / (1e-5 * scale) if scale else 0.0
        print('[layernorm widths] {} {}: max|err| {:.3e}, max|want| {:.3e}, {:.3f} of atol used'.format(
            what, name, (a - b).abs().max().item(), scale, max(need, 0.0)))
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5 * scale), (what, name, (a - b).abs().max().item(), scale)


@pytest.mark.parametrize('rows', [1, 7, 77, 1000, 4096])
@pytest.mark.parametrize('add', [False, True], ids=['plain', 'add'])
@pytest.mark.parametrize('rms', [False, True], ids=['layernorm', 'rms'])
@pytest.mark.parametrize('d', WIDTHS)
def test_forward_and_backward_against_fp64(d, rms, add, rows):
    """rows 1 and 7: fewer rows than a workgroup takes per round; 77 and 1000: a ragged last round."""
    E = _ext()
    gen = torch.Generator().manual_seed(rows + d + int(rms))
    norm = _norm(d, rms, gen)
    x, r, ws, wy = _inputs(rows, d, add, gen)
    want = _fp64(norm, rms, x, r, ws, wy)
    _within(_fp32(norm, rms, x, r, ws, wy, fused=False), want, 'library d={} rows={}'.format(d, rows))
    E.reset_paths()
    got = _fp32(norm, rms, x, r, ws, wy, fused=True)
    assert E.paths_taken('norm') == {('norm', 'kernel'): 1}
    _within(got, want, 'kernel d={} rows={}'.format(d, rows))
    if add:
        assert poison.same_bits(got[2], got[3])                      # one gradient for both summands
    # reproducible: fixed summation order of the row sums and of the parameter gradients
    again = _fp32(norm, rms, x, r, ws, wy, fused=True)
    for a, b, name in zip(again, got, NAMES):
        assert b is None or torch.equal(a, b), name


@pytest.mark.parametrize('rms', [False, True], ids=['layernorm', 'rms'])
@pytest.mark.parametrize('d', WIDTHS)
def test_two_runs_give_the_same_bits(d, rms):
    E = _ext()
    rows = 1000
    gen = torch.Generator().manual_seed(d + 2 * int(rms))
    norm = _norm(d, rms, gen)
    x, r, dy, dskip = _inputs(rows, d, True, gen)
    gamma, beta = norm.weight.detach(), None if rms else norm.bias.detach()

    def run():
        s, y, mean, rstd = E.add_layernorm_forward(x, r, gamma, beta, EPS, rms)
        dx, dgamma, dbeta = E.layernorm_backward(s, dy, gamma, mean, rstd, dskip=dskip, rms=rms)
        return s, y, mean, rstd, dx, dgamma.clone(), dbeta.clone()

    first, second = run(), run()
    for a, b, name in zip(first, second, ('s', 'y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta')):
        assert torch.equal(a, b), name
    assert torch.isfinite(first[2]).all() and torch.isfinite(first[3]).all()
    if rms:
        assert (first[2] == 0).all() and (first[6] == 0).all()


def test_gate_takes_the_new_widths_and_no_others(caplog):
    from naive_gpt import layers
    from naive_gpt.layers.basic import fused_norm
    E = _ext()
    gen = torch.Generator().manual_seed(1)
    E.reset_paths()
    calls = 0
    with caplog.at_level(logging.WARNING, logger='naive_gpt'):
        for d in WIDTHS:
            for rms in (False, True):
                norm = _norm(d, rms, gen)
                x = torch.randn([2, 5, d], generator=gen).to(DEV)
                r = torch.randn([2, 5, d], generator=gen).to(DEV)
                assert fused_norm.usable(norm, x), (d, rms)
                assert E.layernorm_form(d, rms) == (1 if d == 768 or (rms and d == 4096) else E.layernorm_form(d, False))
                s, y = fused_norm.add_norm(norm, x, r)
                calls += 1
                assert torch.equal(s, x + r) and torch.allclose(y, norm(x + r), rtol=1e-4, atol=1e-5)
    # every call on the kernels, none logged as leaving them (this is what the parent of the change fails)
    assert E.paths_taken('norm') == {('norm', 'kernel'): calls}
    assert not [rec for rec in caplog.records if 'norm takes' in rec.getMessage()]
    # 2304 = 9 * 256 stays op by op, with exactly the library's bits
    E.reset_paths()
    for norm in (nn.LayerNorm(2304).to(DEV), layers.LlamaRMSNorm(2304).to(DEV)):
        x = torch.randn([2, 5, 2304], generator=gen).to(DEV)
        r = torch.randn([2, 5, 2304], generator=gen).to(DEV)
        assert not fused_norm.usable(norm, x)
        s, y = fused_norm.add_norm(norm, x, r)
        assert torch.equal(s, x + r) and torch.equal(y, norm(x + r))
    assert E.paths_taken('norm') == {('norm', 'library'): 2}


# ------------------------------------------------------------------------------ norm on load

def _case(rows, d, n, rms, seed):
    """as tests/test_gpu_norm_on_load.py::_case: gaussian activations, rows scaled 2^-12 .. 1"""
    gen = torch.Generator().manual_seed(seed)
    s = torch.randn([rows, d], generator=gen, dtype=torch.float64)
    s = (s * torch.pow(2.0, -torch.randint(0, 13, [rows, 1], generator=gen).double())).float()
    gamma = 1 + 0.2 * torch.randn([d], generator=gen)
    beta = None if rms else 0.1 * torch.randn([d], generator=gen)
    narrow = torch.randn([rows, n], generator=gen) / math.sqrt(rows)
    to = lambda t: None if t is None else t.to(DEV)
    return to(s), to(gamma), to(beta), to(narrow)


@pytest.mark.parametrize('rows', [8192, 1500])
@pytest.mark.parametrize('d,rms', [(768, False), (768, True), (2560, False), (2560, True), (5120, True)])
def test_norm_on_load_equals_the_product_on_the_norm_output(d, rms, rows):
    """The table-gradient product that forms the norm's output on load (ext.tall_tn with `norm`) from the
    statistics these kernels wrote == the product on the y they stored: same bits, three layouts."""
    E = _ext()
    s, gamma, beta, narrow = _case(rows, d, 16, rms, seed=rows + d)
    _, y, mean, rstd = E.add_layernorm_forward(s, None, gamma, beta, EPS, rms)
    norm = (None if rms else mean, rstd, gamma, beta)
    for kw in [{}, {'transposed': True}, {'split16': True}]:
        want = E.tall_tn(y, narrow, **kw)
        got = E.tall_tn(s, narrow, norm=norm, **kw)
        assert got.shape == want.shape and torch.equal(got, want), kw
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0


# ------------------------------------------------------------------------------ poisoned buffers

@pytest.mark.parametrize('d,rms', [(768, False), (2560, False), (4096, False), (5120, False), (2560, True), (5120, True)])
def test_poisoned_outputs_and_partials_change_nothing(d, rms):
    """The shape of test_gpu_poisoned_buffers._layernorm (forward with an addend, backward with a skip
    gradient, 37 rows: fewer than the 512 partial rows' worth, a ragged round) at the new widths: outputs,
    statistics and the partial rows filled before the call leave the bits alone, and the values meet the
    fp64 bound of this file."""
    E = _ext()
    rows = 37
    gen = torch.Generator().manual_seed(22 + d)
    norm = _norm(d, rms, gen)
    x, r, dy, dskip = _inputs(rows, d, True, gen)
    gamma, beta = norm.weight.detach(), None if rms else norm.bias.detach()

    def call():
        s, y, mean, rstd = E.add_layernorm_forward(x, r, gamma, beta, EPS, rms=rms)
        dx, dgamma, dbeta = E.layernorm_backward(s, dy, gamma, mean, rstd, dskip=dskip, rms=rms)
        return s, y, mean, rstd, dx, dgamma, dbeta

    plain = [t.clone() for t in call()]
    for pattern in poison.PATTERNS:
        with poison.poisoned(pattern) as state:
            outs = call()
        assert state.count >= 7 and not state.unclassified
        for a, b, name in zip(outs, plain, ('s', 'y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta')):
            assert torch.isfinite(a).all() and poison.same_bits(a, b), (pattern, name)
    # fp64: y as the forward weight's gradient source, dskip as the sum's own gradient
    s64 = (x.double() + r.double()).requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = None if rms else beta.double().requires_grad_(True)
    if rms:
        y64 = g64 * (s64 * torch.rsqrt(s64.square().mean(dim=-1, keepdim=True) + EPS))
    else:
        y64 = nn.functional.layer_norm(s64, [d], g64, b64, EPS)
    y64.backward(dy.double())
    want = (s64.detach(), y64.detach(), s64.grad + dskip.double(), None, g64.grad, None if rms else b64.grad)
    _within((plain[0], plain[1], plain[4], None, plain[5], plain[6]), want, 'poisoned d={}'.format(d))
    if rms:
        assert (plain[6] == 0).all() and (plain[2] == 0).all()
