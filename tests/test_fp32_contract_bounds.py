"""The fp32 contract's bounds are neither vacuous nor too tight: on the CPU, the input builders and bounds
of tests/fp32_contract.py (the ones test_gpu_fp32_contract.py holds the kernels to) against
  * a plain fp32 torch evaluation of the correct formula: passes, its worst ratios printed;
  * deliberately wrong fp32 evaluations: each one fails.
"""
import pytest
import torch

import exact as X
import fp32_contract as C


def rejected(outputs, refs, name, what):
    """The bound of output `name` rejects `outputs` (the other outputs are not looked at)."""
    with pytest.raises(AssertionError, match='off its bound'):
        X.assert_within(outputs[name], refs[name][0], refs[name][1], 'wrong on purpose: ' + what)


def perturbed(t, every=100):
    """2^-18 relative in 1 % of the elements."""
    t = t.clone()
    t.view(-1)[::every] *= 1 + 2.0 ** -18
    return t


def through(dtype, x):
    """exp evaluated in a 16-bit format: argument and result rounded to it."""
    return x.to(dtype).float().exp().to(dtype).float()


def test_the_helpers_of_the_tier():
    u = 2.0 ** -24
    mag = torch.tensor([1.0, 0.0, 3.0], dtype=torch.float64)
    assert torch.equal(X.fp32_tree_bound(mag, 15), 15 * u / (1 - 15 * u) * mag)
    assert X.fp32_tree_bound(mag, 15)[0] < X.fp32_sum_bound(mag, 5120)[0] / 300      # the point of the depth
    v = torch.tensor([2.0, -4.0], dtype=torch.float64)
    assert torch.equal(X.eval_bound(v, 2), 2 * u * v.abs())
    assert torch.equal(X.eval_bound(v, 2, arg=torch.tensor([-10.0, 3.0])), torch.tensor([12.0, 5.0]) * u * v.abs())
    ref = torch.tensor([1.0, 2.0, 0.0], dtype=torch.float64)
    bound = torch.tensor([1e-6, 1e-6, 0.0], dtype=torch.float64)
    assert X.assert_within(torch.tensor([1.0 + 5e-7, 2.0, 0.0]), ref, bound, 'ok') == pytest.approx(0.5, rel=0.2)
    with pytest.raises(AssertionError, match='element 1 of 3'):
        X.assert_within(torch.tensor([1.0, 2.0 + 1e-5, 0.0]), ref, bound, 'second')
    with pytest.raises(AssertionError, match='element 2 of 3'):                      # bound 0: exact
        X.assert_within(torch.tensor([1.0, 2.0, 1e-30]), ref, bound, 'exact')
    with pytest.raises(AssertionError):
        X.assert_within(torch.tensor([1.0, float('nan'), 0.0]), ref, bound, 'nan')


# ----------------------------------------------------------------------------------- norm kernels

def norm_forward32(inp, rms, variance='two-pass', drop_tail=False):
    x, r, gamma, beta, eps = inp['x'], inp['r'], inp['gamma'], inp['beta'], inp['eps']
    d = x.size(-1)
    s = x + r if r is not None else x
    if rms:
        mean = torch.zeros(s.size(0))
    elif drop_tail:
        mean = s[:, :-4].sum(-1) / d                       # a row reduction that drops its last float4
    else:
        mean = s.mean(-1)
    c = s - mean[:, None]
    var = (c * c).mean(-1) if variance == 'two-pass' else (s * s).mean(-1) - mean * mean
    rstd = (var + eps).rsqrt()
    y = c * rstd[:, None] * gamma
    return dict(s=s, mean=mean, rstd=rstd, y=y + beta if beta is not None else y)


def norm_backward32(inp, s, mean, rstd, rms, skip_rows=None):
    gamma, dy, dskip = inp['gamma'], inp['dy'], inp['dskip']
    xh = (s - (0 if rms else mean[:, None])) * rstd[:, None]
    g = dy * gamma
    c1 = 0 if rms else g.mean(-1, keepdim=True)
    dx = rstd[:, None] * (g - c1 - xh * (g * xh).mean(-1, keepdim=True))
    if dskip is not None:
        dx = dx + dskip
    keep = torch.ones(s.size(0), dtype=torch.bool)
    if skip_rows is not None:
        keep[skip_rows] = False
    return dict(dx=dx, dgamma=(dy * xh)[keep].sum(0), dbeta=torch.zeros_like(gamma) if rms else dy[keep].sum(0))


@pytest.mark.parametrize('d,rms,rows', [(256, False, 37), (256, True, 37), (5120, False, 37), (4096, True, 37),
                                        (768, False, 4096 + 37)])
def test_norm_bounds_take_fp32_and_reject_wrong_evaluations(d, rms, rows):
    inp = C.norm_inputs(d, rows, rms, seed=d + rows + rms)
    refs = C.norm_forward_refs(inp, rms)
    what = '{} d={} rows={}'.format('rms' if rms else 'ln', d, rows)
    fwd = norm_forward32(inp, rms)
    C.check(fwd, refs, 'fp32 ' + what)
    rejected(dict(y=perturbed(fwd['y'])), refs, 'y', 'y perturbed by 2^-18 in 1 %')
    if not rms:
        rejected(norm_forward32(inp, rms, variance='one-pass'), refs, 'rstd', 'one-pass variance')
        rejected(norm_forward32(inp, rms, drop_tail=True), refs, 'mean', 'mean without its last float4')
    brefs = C.norm_backward_refs(inp, fwd['s'], fwd['mean'], fwd['rstd'], rms)
    bwd = norm_backward32(inp, fwd['s'], fwd['mean'], fwd['rstd'], rms)
    C.check(bwd, brefs, 'fp32 ' + what)
    rejected(dict(dx=perturbed(bwd['dx'])), brefs, 'dx', 'dx perturbed by 2^-18 in 1 %')
    # one partial row lost: the rows of workgroup 0 (a wave per row: rows 8 k nparts .. + 7)
    nparts = C.norm_partial_rows(rows)
    lost = [r for r in range(rows) if (r // 8) % nparts == 0]
    assert len(lost) <= max(8, 2 * rows // nparts)
    wrong = norm_backward32(inp, fwd['s'], fwd['mean'], fwd['rstd'], rms, skip_rows=lost)
    rejected(wrong, brefs, 'dgamma', 'dgamma without one partial row')
    if not rms:
        rejected(wrong, brefs, 'dbeta', 'dbeta without one partial row')


# -------------------------------------------------------------------------------------- head loss

def head_loss32(inp, exp=torch.exp):
    logits, V, target = inp['logits'], inp['V'], inp['target']
    z = logits[:, :V]
    counted = target >= 0
    mx = z.max(-1, keepdim=True).values
    e = exp(z - mx)
    total = e.sum(-1, keepdim=True)
    zt = z.gather(1, target.clamp_min(0)[:, None])
    loss = ((total.log() + mx) - zt)[:, 0] * counted
    scale = inp['scale'] * counted[:, None]
    grad = torch.zeros_like(logits)
    grad[:, :V] = e * (scale / total) - torch.zeros_like(z).scatter_(1, target.clamp_min(0)[:, None], 1.0) * scale
    return dict(loss=loss, grad=grad)


@pytest.mark.parametrize('V,ld', [(1001, 1008), (4100, 4100)])
def test_head_loss_bound_takes_fp32_and_rejects_wrong_evaluations(V, ld):
    inp = C.head_loss_inputs(V, ld, seed=V)
    refs = C.head_loss_refs(inp)
    good = head_loss32(inp)
    C.check(good, refs, 'fp32 head loss V={}'.format(V))
    # the kernel's own exponential, as stated: exp2 of the argument times the fp32 constant log2e
    C.check(head_loss32(inp, exp=lambda a: torch.exp2(a * 1.4426950408889634)), refs, 'fp32, exp2(x log2e), head loss V={}'.format(V))
    rejected(head_loss32(inp, exp=lambda a: through(torch.bfloat16, a)), refs, 'grad', 'exp through bf16')
    rejected(head_loss32(inp, exp=lambda a: through(torch.float16, a)), refs, 'grad', 'exp through fp16')
    rejected(dict(grad=perturbed(good['grad'])), refs, 'grad', 'gradient perturbed by 2^-18 in 1 %')

    def short_sum(a):                                     # the row sum loses its last four terms
        e = torch.exp(a)
        e[:, -4:] = 0
        return e
    rejected(head_loss32(inp, exp=short_sum), refs, 'loss', 'row sum without its last float4')


# ---------------------------------------------------------------------------------- sparse softmax

def softmax32(inp, exp=torch.exp, subtract_max=False, drop_tail=False):
    row_of, S = inp['row_of'], inp['S']
    keep = inp['indices'].long() <= row_of
    v = inp['values']
    if subtract_max:
        top = torch.full([v.size(0), S], -1e30).scatter_reduce(1, row_of.expand_as(v), torch.where(keep, v, -1e30),
                                                               'amax')
        v = v - top[:, row_of]
    e = torch.where(keep, exp(v), 0.0)
    part = e.clone()
    if drop_tail:
        end = inp['indptr'][1:].long()
        last4 = (end[row_of] - torch.arange(inp['nnz'])) <= 4
        part[:, last4] = 0
    total = torch.zeros([v.size(0), S]).index_add_(1, row_of, part).clamp_min(1e-9)
    return dict(y=e * (1.0 / total)[:, row_of])


def softmax_backward32(inp, y, clamped=None):
    row_of, S = inp['row_of'], inp['S']
    keep = inp['indices'].long() <= row_of
    y = torch.where(keep, y, 0.0)
    c = torch.zeros([y.size(0), S]).index_add_(1, row_of, y * inp['dy']).clamp_min(1e-9)
    grad = y * (inp['dy'] - c[:, row_of])
    if clamped is not None:
        grad = torch.where(clamped.abs() < inp['clamp'], grad * inp['scale'], 0.0)
    return dict(grad=grad)


@pytest.mark.parametrize('kind,causal', [('z16', True), ('z64', False), ('ragged', False)])
def test_softmax_bounds_take_fp32_and_reject_wrong_evaluations(kind, causal):
    inp = C.softmax_inputs(kind, causal, seed=len(kind) + causal)
    refs = C.softmax_forward_refs(inp)
    what = 'softmax {} causal={}'.format(kind, causal)
    good = softmax32(inp)
    C.check(good, refs, 'fp32 ' + what)
    rejected(softmax32(inp, exp=lambda a: through(torch.bfloat16, a)), refs, 'y', 'exp through bf16')
    rejected(softmax32(inp, exp=lambda a: through(torch.float16, a)), refs, 'y', 'exp through fp16')
    rejected(softmax32(inp, subtract_max=True), refs, 'y', 'max subtracted: the rows under the floor differ')
    rejected(softmax32(inp, drop_tail=True), refs, 'y', 'row sum without its last four terms')
    rejected(dict(y=perturbed(good['y'])), refs, 'y', 'y perturbed by 2^-18 in 1 %')
    for clamped in (None, C.softmax_clamped_scores(inp)):
        brefs = C.softmax_backward_refs(inp, good['y'], clamped=clamped)
        back = softmax_backward32(inp, good['y'], clamped=clamped)
        C.check(back, brefs, 'fp32 ' + what + ' backward' + (', clamped' if clamped is not None else ''))
        rejected(dict(grad=perturbed(back['grad'], every=7)), brefs, 'grad', 'gradient perturbed by 2^-18')


# ------------------------------------------------------------------------------------ elementwise

def swiglu32(inp, exp=torch.exp):
    g, s, dh = inp['g'], inp['s'], inp['dh']
    sg = 1.0 / (1.0 + exp(-g))
    silu = g / (1.0 + exp(-g))
    h = silu * s
    dg = dh * s * (sg * (1.0 + g * (1.0 - sg)))
    ds = dh * silu
    return dict(h=h, dg=dg, ds=ds, dot_h=(dh * h).sum(1), dot_g=(dg * g).sum(1), dot_s=(ds * s).sum(1))


def test_swiglu_bounds_take_fp32_and_reject_wrong_evaluations():
    inp = C.swiglu_inputs(200, 520, seed=3)
    good = swiglu32(inp)
    refs = dict(C.swiglu_forward_refs(inp), **C.swiglu_backward_refs(inp, good['dg'], good['ds']))
    C.check(good, refs, 'fp32 swiglu')
    wrong = swiglu32(inp, exp=lambda a: through(torch.float16, a.clamp(-10, 10)))
    for name in ('h', 'dg', 'ds', 'dot_h'):
        rejected(wrong, refs, name, 'exp through fp16')
        if name != 'dot_h':        # (2^-18 of a row dot is inside the rounding of its 520 cancelling terms)
            rejected({name: perturbed(good[name], every=3)}, refs, name, 'perturbed by 2^-18')
    short = dict(good, dot_g=(good['dg'] * inp['g'])[:, :-4].sum(1))
    rejected(short, refs, 'dot_g', 'row dot without its last float4')


@pytest.mark.parametrize('transpose', [False, True])
def test_rotary_bound_takes_fp32_and_rejects_wrong_evaluations(transpose):
    inp = C.rotary_inputs(3, seed=5)
    refs = C.rotary_refs(inp, 2, transpose)
    S, E = inp['parts'][0].size(1), inp['parts'][0].size(3)
    c, s = inp['cos'][:S].view(1, S, 1, E), inp['sin'][:S].view(1, S, 1, E)
    half = E // 2

    def rotate(x, sign=1.0):
        lo, hi = x[..., :half], x[..., half:]
        if not transpose:
            return c * x + sign * s * torch.cat([-hi, lo], -1)
        return c * x + sign * torch.cat([s[..., half:] * hi, -s[..., :half] * lo], -1)
    good = torch.stack([rotate(inp['parts'][0]), rotate(inp['parts'][1]), inp['parts'][2]])
    C.check(dict(out=good), refs, 'fp32 rotary transpose={}'.format(transpose))
    rejected(dict(out=perturbed(good)), refs, 'out', 'perturbed by 2^-18 in 1 %')
    # the forward formula where the adjoint is asked for (and the other way round)
    other = C.rotary_refs(inp, 2, not transpose)
    rejected(dict(out=good), other, 'out', 'the adjoint and the forward exchanged')
    rejected(dict(out=torch.stack([rotate(inp['parts'][0]), rotate(inp['parts'][1]), inp['parts'][2] * (1 + 2.0 ** -23)])),
             refs, 'out', 'a copied part that is not bit-exact')


# ---------------------------------------------------------------------------- routing, sparse, PQ

def test_routing_bounds_take_fp32_and_reject_wrong_evaluations():
    inp = C.route_inputs(1000, 4, seed=6)
    ref, bound = C.route_prob_refs(inp)
    v = inp['logits'][:, :4] + inp['bias']
    X.assert_within(1.0 / (1.0 + torch.exp(-v)), ref, bound, 'fp32 router sigmoid')
    rejected(dict(p=1.0 / (1.0 + through(torch.float16, -v.clamp(-10, 10)))), dict(p=(ref, bound)), 'p', 'exp through fp16')
    rejected(dict(p=perturbed(1.0 / (1.0 + torch.exp(-v)))), dict(p=(ref, bound)), 'p', 'perturbed by 2^-18 in 1 %')
    token, block, pos = C.route_selection(inp['prob'].double(), 2)
    y = inp['prob']
    for prob in (None, y):
        refs = C.route_backward_refs(inp, token, block, prob)
        name = next(iter(refs))
        out = torch.zeros(1000, 4)
        out[token, block] = inp['scale'] * inp['dcoeff']
        out = out if prob is None else (out * (1.0 - y)) * y
        C.check({name: out}, refs, 'fp32 route_coeff_backward')
        rejected({name: perturbed(out, every=3)}, refs, name, 'perturbed by 2^-18')
    f = C.ffn_coeff_inputs(1000, 500, 6, 16, seed=2)
    refs = C.ffn_coeff_refs(f)
    tok = f['token'].long()

    def coeff_grad(w):
        num = f['dot_main'][:, :w].sum(1) + f['dot_act'].sum(1) - (f['du'] * f['u'][tok]).sum(1) - (f['dzt'][tok] * f['z']).sum(1)
        return dict(out=num / torch.maximum(f['coeff'], torch.tensor(f['floor'])))
    C.check(coeff_grad(6), refs, 'fp32 ffn_coeff_grad')
    rejected(coeff_grad(5), refs, 'out', 'a sum without its last term')
    e = C.embedding_inputs(4096, 16, 5000, seed=3)
    refs = C.embedding_refs(e)
    good = torch.zeros(5000, 16, dtype=torch.float64).index_add_(0, e['ids'], e['grad'].double()).float()
    C.check(dict(out=good), refs, 'embedding rows, summed in fp64')
    rejected(dict(out=torch.zeros(5000, 16).index_add_(0, e['ids'], e['grad'])), refs, 'out', '3000 rows summed in fp32')
    c = C.combine_inputs(1000, 2, 24, 4, seed=4)
    good = c['bias'] + c['rows'][c['pos'].long()].sum(1) + c['side'] @ c['side_weight']
    C.check(dict(out=good), C.combine_refs(c, True), 'fp32 rows_combine')
    rejected(dict(out=good), C.combine_refs(c, False), 'out', 'the side product where none is asked')


@pytest.mark.parametrize('B,S,E,kind', [(3, 96, 20, 'z16'), (3, 96, 64, 'ragged'), (2, 1024, 64, 'z16')])
def test_sparse_bounds_take_fp32_and_reject_wrong_evaluations(B, S, E, kind):
    inp = C.sparse_inputs(B, S, E, kind, seed=B + E)
    bi = torch.arange(B)[:, None]
    cols, rows = inp['indices'].long(), inp['row_of'].expand(B, inp['nnz'])
    prod = inp['q'][:, inp['row_of']] * inp['k'][bi, cols]
    refs = C.sddmm_refs(inp, 0.5, 10.0)
    C.check(dict(out=(prod.sum(-1) * 0.5).clamp(-10, 10)), refs, 'fp32 sddmm')
    rejected(dict(out=(prod[..., :-4].sum(-1) * 0.5).clamp(-10, 10)), refs, 'out', 'dot without its last float4')
    rejected(dict(out=perturbed((prod.sum(-1) * 0.5).clamp(-10, 10))), refs, 'out', 'perturbed by 2^-18 in 1 %')
    for transposed in (False, True):
        refs = C.spmm_refs(inp, transposed)
        src, dst = (rows, cols) if transposed else (cols, rows)
        terms = inp['values'][..., None] * inp['x'][bi, src]
        at = dst[..., None].expand(B, inp['nnz'], E)
        C.check(dict(y=torch.zeros(B, S, E).scatter_add_(1, at, terms)), refs, 'fp32 spmm T={}'.format(transposed))
        short = terms.clone()
        short[:, ::97] = 0                                 # entries lost
        rejected(dict(y=torch.zeros(B, S, E).scatter_add_(1, at, short)), refs, 'y', 'entries lost')


@pytest.mark.parametrize('Z,causal', [(16, True), (64, False)])
def test_attention_chain_bound_takes_fp32_and_rejects_wrong_evaluations(Z, causal):
    N, H, S = 1, 4, 128
    inp = C.attention_inputs(N, H, S, Z, causal, seed=Z)
    refs = C.attention_forward_refs(inp)
    B = N * H
    q, k, v = (t.transpose(1, 2).reshape(B, S, 64) for t in (inp['q'], inp['k'], inp['v']))
    cols = inp['indices'].long().view(B, S, Z)
    keep = cols <= torch.arange(S).view(1, S, 1)

    def forward(exp=torch.exp):
        s = ((q @ k.transpose(1, 2)).gather(2, cols) * inp['scale']).clamp(-10, 10)
        e = torch.where(keep, exp(s), 0.0)
        attn = e * (1.0 / e.sum(-1, keepdim=True).clamp_min(1e-9))
        y = torch.zeros(B, S, S).scatter_add_(2, cols, attn) @ v
        return dict(scores=s.view(B, -1), attn=attn.view(B, -1), y=y)
    good = forward()
    C.check(good, refs, 'fp32 attention chain Z={}'.format(Z))
    rejected(forward(exp=lambda a: through(torch.bfloat16, a)), refs, 'attn', 'exp through bf16')
    rejected(forward(exp=lambda a: through(torch.float16, a)), refs, 'y', 'exp through fp16')
    # (2^-18 of a forward output is inside what the 64-term dot products may lose -- the score's error is in
    # the exponent of every probability; the perturbed result of this group is grad_raw, below)
    # (no max-subtraction case: the clamp keeps every live score >= -10, so only a fully masked row falls
    # under the 1e-9 floor, and that row is 0 either way; the sparse softmax's test has the case)
    brefs = C.attention_backward_refs(inp, good['scores'], good['attn'])
    p = good['attn'].view(B, S, Z) * keep
    dP = (inp['dy'] @ v.transpose(1, 2)).gather(2, cols)
    c = (p * dP).sum(-1, keepdim=True).clamp_min(1e-9)
    dS = torch.where(good['scores'].view(B, S, Z).abs() < 10, p * (dP - c) * inp['scale'], 0.0)
    gq = (torch.zeros(B, S, S).scatter_add_(2, cols, dS) @ k).view(N, H, S, 64).transpose(1, 2)
    C.check(dict(grad_raw=dS.view(B, -1), grad_q=gq), brefs, 'fp32 attention backward Z={}'.format(Z))
    rejected(dict(grad_raw=perturbed(dS.view(B, -1), every=3)), brefs, 'grad_raw', 'perturbed by 2^-18')


def pq32(inp, accumulate=False, exact_division=True, lose_block=False):
    """The PQ loss and its gradients in fp32 torch, from the formulas of pq_loss.hip's header."""
    z, table, parts = inp['z'], inp['table'], inp['parts']
    M, Cw, D = table.shape
    sub = z.view(-1, D)
    total = sub.size(0)
    count = total // parts * D
    W = table[torch.arange(total) % M]
    d = (sub[:, None, :] - W).abs().sum(-1)
    best = d.argmin(-1)
    dc = d.clamp_min(1e-5)
    softu = dc.gather(1, best[:, None]) / dc
    soft = softu / softu.sum(-1, keepdim=True)
    zq = W[torch.arange(total), best]
    zw = (soft[..., None] * W).sum(1)
    e1, e2 = zw - zq, sub - zq
    loss = (e1 * e1 + e2 * e2).sum() / count
    g2 = 2 * inp['grad_loss'] / count
    gzw, e2g = g2 * e1, g2 * e2
    gs = (gzw[:, None, :] * W).sum(-1)
    ga = soft * (gs - (soft * gs).sum(-1, keepdim=True))
    gd = torch.where(d >= 1e-5, -ga / dc, 0.0)
    s = torch.where(W >= sub[:, None, :], 1.0, -1.0)
    gz = e2g - (s * gd[..., None]).sum(1)
    if accumulate:
        gz = gz + inp['prior'].view(-1, D)
    onehot = torch.zeros_like(soft).scatter_(1, best[:, None], 1.0)
    terms = soft[..., None] * gzw[:, None, :] + onehot[..., None] * (-gzw - e2g)[:, None, :] + s * gd[..., None]
    if lose_block:
        terms[:128 * M] = 0                                # one workgroup's sub-vectors
    return dict(loss=loss, grad_z=gz.view(z.shape), grad_weight=terms.view(total // M, M, Cw, D).sum(0))


@pytest.mark.parametrize('M,parts', [(8, 1), (10, 2)])
def test_pq_bounds_take_fp32_and_reject_wrong_evaluations(M, parts):
    inp = C.pq_inputs(M, seed=M, parts=parts)
    refs = C.pq_refs(inp, accumulate=parts == 2)
    good = pq32(inp, accumulate=parts == 2)
    C.check(good, refs, 'fp32 pq_loss M={}'.format(M))
    rejected(pq32(inp, accumulate=parts == 2, lose_block=True), refs, 'grad_weight', 'one workgroup\'s share lost')
    rejected(dict(loss=good['loss'] * (1 + 2.0 ** -16)), refs, 'loss', 'loss off by 2^-16')
    rejected(dict(grad_z=perturbed(good['grad_z'] * 1.0, every=1)), refs, 'grad_z', 'grad_z perturbed by 2^-18')
    D = inp['table'].size(-1)
    query = inp['z'].view(-1, M, D).transpose(0, 1).contiguous()
    go = torch.randn([M, query.size(1), 16], generator=torch.Generator().manual_seed(M))
    crefs = C.cdist_backward_refs(query, inp['table'], go)
    s = torch.where(query[:, :, None, :] > inp['table'][:, None, :, :], 1.0, -1.0)
    C.check(dict(grad_query=(s * go[..., None]).sum(2), grad_table=-(s * go[..., None]).sum(1)), crefs, 'fp32 cdist_backward')
    s_wrong = torch.where(query[:, :, None, :] >= inp['table'][:, None, :, :], 1.0, -1.0)      # the tie the other way
    rejected(dict(grad_query=(s_wrong * go[..., None]).sum(2)), crefs, 'grad_query', 'sign at equality')
