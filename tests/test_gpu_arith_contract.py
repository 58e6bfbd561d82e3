"""GPU tier, contract: gaussian inputs against the arithmetic each kernel states, element by element.

fp32 split kernels: |got - exact| <= split_bound (tests/exact.py: c_K sum_k |a_k||b_k|, derived there).
bf16-storing kernels: the stored value is RNE of the exact result, except within a band around a rounding
midpoint that the kernel's own fp32 arithmetic may cross (assert_once_rounded); every band is derived
below from fp32 accumulation and the activation's evaluation.  The rows of `a` are scaled by 2^-12 .. 1 so
that many outputs are small against the tensor's maximum: a bar relative to max|want| would not see
them.  Each bf16 test prints the share of elements that fell in its band ("[band]" lines, with -s).

The matrix-core attention kernels (fp32 and bf16 storage, forward and backward) are bounded per element
from the magnitudes along their chain (derived above test_attention_mfma_within_the_chain_bound).
"""
import math

import pytest
import torch

import exact as X

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24
# fp32 evaluation of GELU (erff) / SiLU (__expf) at an fp32 input s: erff and the exp are within a few
# ulp of their results, and 1 + erf(.) / 1 + exp(.) cancel at most to an absolute error of ~2 ulp(1)
# times |s| / 2; the products after them add one rounding each.  2^-20 (16 ulp) of |act(s)| + |s| covers
# all of it with room.
ACT_EVAL = 2.0 ** -20


def _act64(act, s):
    if act == 'gelu':
        return 0.5 * s * (1 + torch.erf(s / math.sqrt(2)))
    return s * torch.sigmoid(s)


def _act_slope_max(act):
    return 1.13 if act == 'gelu' else 1.1        # max |act'| over the reals


def _ext():
    from naive_gpt import ext as E
    return E


def _band_line(what, n_band, total):
    share = n_band / max(total, 1)
    print('[band] {}: {} of {} ({:.3%})'.format(what, n_band, total, share))
    return share


def _inputs(gen, P, K, N, G):
    a = torch.randn([P, K], generator=gen, dtype=torch.float64)
    a = a * torch.pow(2.0, -torch.randint(0, 13, [P, 1], generator=gen).double())      # small rows
    w = torch.randn([G, N, K], generator=gen, dtype=torch.float64) / math.sqrt(K)
    return a.float(), w.float()


@pytest.mark.parametrize('act', ['gelu', 'silu'])
@pytest.mark.parametrize('path', ['register', 'image'])
def test_split_gemm_gelu_silu_within_the_split_bound(act, path):
    E = _ext()
    gen = torch.Generator().manual_seed(len(act) + len(path))
    sizes = [0, 300, 129, 1, 0, 270]
    G, P, K, N = len(sizes), sum(sizes), 256, 192
    a, w = _inputs(gen, P, K, N, G)
    bias = torch.randn([G, N], generator=gen) * 0.01
    rowscale = torch.rand([P], generator=gen) + 0.5
    cuts = torch.tensor([0] + sizes).cumsum(0)
    g_of = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    wg = w.double()[g_of]                                                      # [P, N, K]
    v = rowscale.double()[:, None] * (torch.einsum('pk,pnk->pn', a.double(), wg) + bias.double()[g_of])
    mag = torch.einsum('pk,pnk->pn', a.double().abs(), wg.abs()) + bias.double().abs()[g_of]
    # split_bound covers the k-loop (3K products) and the bias addition; the rowscale product adds one
    # rounding of the result
    bound = rowscale.double()[:, None] * X.split_bound(mag, K, extra_terms=1) + U * v.abs()
    kw = {}
    if path == 'image':
        kw = dict(a_image=E.split_bf16(a.to(DEV)), w_image=E.split_bf16(w.view(G * N, K).to(DEV)))
    out, pre = E.grouped_gemm_fused(a.to(DEV), w.view(G * N, K).to(DEV), cuts.int().to(DEV), G, N, K, N * K, K, 1, P,
                                    bias=bias.to(DEV), rowscale=rowscale.to(DEV), epilogue=E.EPI_ACT,
                                    activation=E.ACT_GELU if act == 'gelu' else E.ACT_SILU, keep_preact=True, **kw)
    assert E.LAST_GEMM_PATH == path
    err = (pre.double().cpu() - v).abs()
    small = v.abs() < 1e-3 * v.abs().max()
    assert small.float().mean() > 0.1                         # the bound is per element, not per max
    assert (err <= bound).all(), 'pre-activation off the split bound: worst ratio {:.3f}'.format(
        float((err / bound).max()))
    p64 = pre.double().cpu()
    assert ((out.double().cpu() - _act64(act, p64)).abs() <= ACT_EVAL * (_act64(act, p64).abs() + p64.abs())).all()


@pytest.mark.parametrize('n', [16, 48])
def test_split_lora_down_and_tall_tn_within_the_split_bound(n):
    E = _ext()
    gen = torch.Generator().manual_seed(n)
    rows, K = 1500, 256
    x, _ = _inputs(gen, rows, K, 1, 1)
    t = torch.randn([K, n], generator=gen)
    u = E.lora_down(x.to(DEV), t.to(DEV))
    want = x.double() @ t.double()
    bound = X.split_bound(x.double().abs() @ t.double().abs(), K)
    assert ((u.double().cpu() - want).abs() <= bound).all()
    # tall_tn: contraction over 1500 rows in chunks, then an in-order fp32 sum of the chunk partials
    narrow = torch.randn([rows, n], generator=gen)
    got = E.tall_tn(x.to(DEV), narrow.to(DEV))[0]
    want = x.double().T @ narrow.double()
    bound = X.split_bound(x.double().abs().T @ narrow.double().abs(), rows)
    assert ((got.double().cpu() - want).abs() <= bound).all()


def test_split_wgrad_within_the_split_bound():
    E = _ext()
    gen = torch.Generator().manual_seed(5)
    sizes = [0, 1100, 1, 300]
    G, P, n, k = len(sizes), sum(sizes), 64, 96
    g_op, _ = _inputs(gen, P, n, 1, 1)
    a_op = torch.randn([P, k], generator=gen)
    rs = torch.rand([P], generator=gen) + 0.5
    out, _ = E.grouped_gemm_wgrad(g_op.to(DEV), a_op.to(DEV), torch.tensor([0] + sizes).cumsum(0).int().to(DEV),
                                  (n, k, n * k, k, 1), P, rowscale=rs.to(DEV))
    cuts = [0] + torch.tensor(sizes).cumsum(0).tolist()
    for g in range(G):
        sl = slice(cuts[g], cuts[g + 1])
        gg = g_op[sl].double() * rs[sl, None].double()
        want = gg.T @ a_op[sl].double()
        # rowscale * G is one more rounding per product (2^-24), then the split of the product
        bound = X.split_bound(gg.abs().T @ a_op[sl].double().abs(), cuts[g + 1] - cuts[g], extra_terms=2)
        assert ((out.view(G, n, k)[g].double().cpu() - want).abs() <= bound * (1 + 2 * U)).all(), g


@pytest.mark.parametrize('act', ['gelu', 'silu'])
def test_bf16_gemm_gelu_silu_is_rounded_once(act):
    """fp32 accumulation of exact products: |v_fp32 - v| <= gamma_(K + 2) (sum |a||w| + |bias|) rowscale
    (K additions, the bias, the rowscale product); the activation moves that by <= max|act'| times it,
    and its own evaluation by ACT_EVAL: the band around a midpoint."""
    E = _ext()
    gen = torch.Generator().manual_seed(len(act))
    sizes = [0, 300, 129, 1, 0, 270]
    G, P, K, N = len(sizes), sum(sizes), 128, 128
    a, w = _inputs(gen, P, K, N, G)
    a, w = a.bfloat16(), w.bfloat16()
    bias = (torch.randn([G, N], generator=gen) * 0.01).bfloat16()
    rowscale = torch.rand([P], generator=gen) + 0.5
    g_of = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    wg = w.double()[g_of]
    v = rowscale.double()[:, None] * (torch.einsum('pk,pnk->pn', a.double(), wg) + bias.double()[g_of])
    mag = rowscale.double()[:, None] * (torch.einsum('pk,pnk->pn', a.double().abs(), wg.abs())
                                        + bias.double().abs()[g_of])
    dv = X.fp32_sum_bound(mag, K + 2)
    want = _act64(act, v)
    band = _act_slope_max(act) * dv + ACT_EVAL * (want.abs() + v.abs())
    out, pre = E.grouped_gemm_bf16(a.to(DEV), w.view(G * N, K).to(DEV), torch.tensor([0] + sizes).cumsum(0).int().to(DEV),
                                   G, N, K, N * K, K, 1, bias=bias.to(DEV), rowscale=rowscale.to(DEV),
                                   epilogue=E.EPI_ACT, activation=E.ACT_GELU if act == 'gelu' else E.ACT_SILU,
                                   keep_preact=True)
    nb, tot = X.assert_once_rounded(pre, v, dv, 'bf16 pre-activation ' + act)
    # measured: ~5.5 % -- gamma_(K + 2) is the worst case of the accumulation, not its typical error
    assert _band_line('grouped_gemm_bf16 pre-activation ' + act, nb, tot) < 0.08
    nb, tot = X.assert_once_rounded(out, want, band, 'bf16 ' + act)
    # measured: ~11 % at K = 128 -- the worst-case gamma_(K + 2) of the accumulation, not its typical error
    assert _band_line("grouped_gemm_bf16 " + act, nb, tot) < 0.15


def test_swiglu_bf16_is_rounded_once():
    E = _ext()
    gen = torch.Generator().manual_seed(8)
    rows, n = 300, 256
    scale = torch.pow(2.0, -torch.randint(0, 13, [rows, 1], generator=gen).float())
    g = (torch.randn([rows, n], generator=gen) * 3).bfloat16()
    s = (torch.randn([rows, n], generator=gen) * scale).bfloat16()
    dh = (torch.randn([rows, n], generator=gen) * scale).bfloat16()
    g64, s64, dh64 = g.double(), s.double(), dh.double()
    sg = torch.sigmoid(g64)
    silu = g64 * sg
    # h = silu(g) * s in fp32: silu's evaluation (ACT_EVAL) and one product rounding
    h = silu * s64
    band_h = (ACT_EVAL * (silu.abs() + g64.abs()) + U * silu.abs()) * s64.abs() + U * h.abs()
    got_h = E.swiglu_forward_bf16(g.to(DEV), s.to(DEV))
    _band_line('swiglu_forward_bf16', *X.assert_once_rounded(got_h, h, band_h, 'swiglu_forward_bf16'))
    # dg = dh s silu'(g), silu'(g) = sg (1 + g (1 - sg)): sg to ACT_EVAL relative, (1 - sg) to ACT_EVAL
    # absolute, times (1 + |g|); ds = dh silu(g)
    dg = dh64 * s64 * sg * (1 + g64 * (1 - sg))
    ds = dh64 * silu
    band_dg = ACT_EVAL * (dh64 * s64).abs() * (1 + 2 * g64.abs()) + 4 * U * dg.abs()
    band_ds = ACT_EVAL * dh64.abs() * (silu.abs() + g64.abs()) + 2 * U * ds.abs()
    got_dg, got_ds = E.swiglu_backward_bf16(dh.to(DEV), g.to(DEV), s.to(DEV))
    for got, want, band, what in ((got_dg, dg, band_dg, 'swiglu_backward_bf16 dg'),
                                  (got_ds, ds, band_ds, 'swiglu_backward_bf16 ds')):
        _band_line(what, *X.assert_once_rounded(got, want, band, what))
    # the dots variant: the same stored values, and row dots of the STORED values summed in fp32
    dg2, ds2, dot_h, dot_g, dot_s = E.swiglu_backward_dots_bf16(dh.to(DEV), g.to(DEV), s.to(DEV))
    assert torch.equal(dg2, got_dg) and torch.equal(ds2, got_ds)
    for dot, x, y, what in ((dot_h, dh64, got_h.double().cpu(), 'dot_h'), (dot_g, dg2.double().cpu(), g64, 'dot_g'),
                            (dot_s, ds2.double().cpu(), s64, 'dot_s')):
        want = (x * y).sum(1)
        bound = X.fp32_sum_bound((x * y).abs().sum(1), n)
        assert ((dot.double().cpu() - want).abs() <= bound).all(), what


# ------------------------------------------------------------------------------ attention (MFMA)
#
# The chain of spt_attention_mfma_forward / _backward (include/spt_hip.h), per slice, in fp64 on dense
# [S, S] cell arrays (M: the CSR multiplicity of every cell), with the error each step can add, first
# order, from the magnitudes of its own operands:
#   d = q k^T           split product over E:  |dd| <= c_E sum_e |q_e||k_e|                 (split_bound)
#   p = exp(scale d)    via exp2(d * fl(scale log2e)): two roundings of the argument (3 u |s|), the exp2
#                       itself within 2^-21 relative, and scale |dd|:  |dp| <= p * delta (1 + delta)
#   num = (M p) V       split product over <= S keys: split_bound(sum M p |v|, S) + sum M |dp| |v|
#   R = sum M p         fp32 sums (<= 3 S additions, whatever the order) + sum M |dp|
#   y = num / R         |dy| <= (|dnum| + |y| |dR|) / (R - |dR|) + 2 u |y|
# Backward, on the y and row_sum it is GIVEN (the forward's stored ones):
#   P = M p / R         |dP| <= M |dp| / R + 3 u P (the reciprocal and the folded factors)
#   dP = dy v^T         split over E, + 2 u of the magnitudes (dy is scaled by scale / R before the split)
#   delta = max(1e-9, dy . y)  fp32 sum over E (max is 1-Lipschitz)
#   dS = scale P (dP - delta)       |ddS| <= scale (|dP| |dP - delta| + P (|ddP| + |ddelta|)) + 3 u |dS|
#   grad_q = dS k, grad_k = dS^T q, grad_v = P^T dy: split over S + the operand's error times the other.
# Scores stay far inside the clamp (asserted), so its mask passes every cell.  A factor 1 + 2^-10 covers
# the second-order terms.  bf16 storage computes the same chain on the widened inputs (bf16 q, k, v are
# exact split operands: the fp32 bound is an upper bound) and rounds each stored result once: the same
# bounds are its bands.
ATT_SHAPES = [(1, 4, 256, 32, 64), (1, 2, 160, 16, 128)]          # (N, H, S, Z, d_head)


def _attention_inputs(N, H, S, Z, E, seed, bf16):
    from test_gpu_fused_attention import causal_indices
    gen = torch.Generator().manual_seed(seed)
    B = N * H
    q, k, v = [torch.randn([N, S, H, E], generator=gen) for _ in range(3)]
    v = v * torch.pow(2.0, -torch.randint(0, 13, [N, S, H, 1], generator=gen).float())   # small rows of y
    dy = torch.randn([B, S, E], generator=gen) * torch.pow(2.0, -torch.randint(0, 13, [B, S, 1], generator=gen).float())
    if bf16:
        q, k, v, dy = [t.bfloat16() for t in (q, k, v, dy)]
    indices = causal_indices(B, S, Z, gen)
    M = torch.zeros([B, S, S], dtype=torch.float64)
    M.scatter_add_(2, indices.view(B, S, Z).long(), torch.ones([B, S, Z], dtype=torch.float64))
    return q, k, v, dy, indices, M


def _flat(t, B, S, E):
    return t.transpose(1, 2).reshape(B, S, E).double()


def _attention_chain(q, k, v, M, scale):
    """fp64 forward chain and its per-element error bounds (see above)."""
    S, E = q.size(1), q.size(2)
    s = scale * (q @ k.transpose(1, 2))
    assert float((s * (M > 0)).abs().max()) < 9.0                   # the clamp (10) never acts
    dd = X.split_bound(q.abs() @ k.abs().transpose(1, 2), E, extra_terms=2)    # (+ the scaled q's rounding)
    delta = scale * dd + 3 * U * s.abs() + 2.0 ** -21
    p = torch.exp(s)
    dp = p * delta * (1 + delta)
    Mp, Mdp = M * p, M * dp
    R = Mp.sum(-1)
    dR = X.fp32_sum_bound(R, 3 * S) + Mdp.sum(-1) + U * R
    num = Mp @ v
    dnum = X.split_bound(Mp @ v.abs(), S) + Mdp @ v.abs() + U * (Mp @ v.abs())
    y = num / R[..., None]
    dy_bound = (dnum + y.abs() * dR[..., None]) / (R - dR)[..., None] + 2 * U * y.abs()
    return dict(Mp=Mp, Mdp=Mdp, R=R, dR=dR, y=y, dy=dy_bound * (1 + 2.0 ** -10))


def _attention_backward_chain(q, k, v, y_g, R_g, dy, c, scale):
    S, E = q.size(1), q.size(2)
    P = c['Mp'] / R_g[..., None]
    dPr = c['Mdp'] / R_g[..., None] + 3 * U * P
    dP = dy @ v.transpose(1, 2)
    mag_dP = dy.abs() @ v.abs().transpose(1, 2)
    ddP = X.split_bound(mag_dP, E) + 2 * U * mag_dP
    rowdot = (dy * y_g).sum(-1)
    delta = rowdot.clamp_min(1e-9)
    ddelta = X.fp32_sum_bound((dy * y_g).abs().sum(-1), E) + U * delta
    gap = dP - delta[..., None]
    dS = scale * P * gap
    ddS = scale * (dPr * gap.abs() + P * (ddP + ddelta[..., None])) + 3 * U * dS.abs()
    out = {}
    for name, w, dw, other in (('q', dS, ddS, k), ('k', dS.transpose(1, 2), ddS.transpose(1, 2), q),
                               ('v', P.transpose(1, 2), dPr.transpose(1, 2), dy)):
        bound = X.split_bound(w.abs() @ other.abs(), S) + dw @ other.abs()
        out[name] = (w @ other, bound * (1 + 2.0 ** -10))
    return out


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('N,H,S,Z,E', ATT_SHAPES)
def test_attention_mfma_within_the_chain_bound(N, H, S, Z, E, bf16):
    E_ = _ext()
    B = N * H
    q, k, v, dy, indices, M = _attention_inputs(N, H, S, Z, E, seed=S + E + bf16, bf16=bf16)
    assert E_.attention_mfma_supported(S, E, S * Z)
    scale = E ** -0.5
    tiles = E_.attention_mfma_prepare(indices.cuda(), S)
    y, row_sum = E_.attention_mfma_forward(tiles, q.cuda(), k.cuda(), v.cuda(), scale, 10.0)
    qf, kf, vf = (_flat(t, B, S, E) for t in (q, k, v))
    c = _attention_chain(qf, kf, vf, M, scale)
    err_r = (row_sum.double().cpu() - c['R']).abs()
    assert (err_r <= c['dR']).all(), 'row_sum off its bound: worst ratio {:.3f}'.format(float((err_r / c['dR']).max()))
    tag = 'bf16' if bf16 else 'fp32'
    if bf16:
        _band_line('attention_mfma_forward_bf16 y S={} E={}'.format(S, E),
                   *X.assert_once_rounded(y.cpu(), c['y'], c['dy'], 'attention bf16 y'))
    else:
        err = (y.double().cpu() - c['y']).abs()
        assert (err <= c['dy']).all(), 'y off its bound: worst ratio {:.3f}'.format(float((err / c['dy']).max()))
    # the backward, on the y / row_sum the forward returned (as autograd hands them over)
    gq, gk, gv = E_.attention_mfma_backward(tiles, q.cuda(), k.cuda(), v.cuda(), y, dy.cuda(), row_sum, scale, 10.0)
    want = _attention_backward_chain(qf, kf, vf, y.double().cpu(), row_sum.double().cpu(), dy.double(), c, scale)
    for name, got in (('q', gq), ('k', gk), ('v', gv)):
        val, bound = want[name]
        got = _flat(got.cpu(), B, S, E) if not bf16 else got.cpu().transpose(1, 2).reshape(B, S, E)
        if bf16:
            _band_line('attention_mfma_backward_bf16 grad_{} S={} E={}'.format(name, S, E),
                       *X.assert_once_rounded(got, val, bound, 'attention bf16 grad_' + name))
        else:
            err = (got - val).abs()
            assert (err <= bound).all(), '{} grad_{} off its bound: worst ratio {:.3f}'.format(
                tag, name, float((err / bound).max()))
