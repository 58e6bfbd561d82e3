"""GPU tier, fp32 contract: the vector-ALU kernels against fp64, element by element.

Every reference is torch fp64 on the CPU and every bound is derived from the kernel's stated arithmetic:
both live in tests/fp32_contract.py, beside the input builders, because test_fp32_contract_bounds.py
runs the same ones against fp32 CPU evaluations (the correct formula passes, wrong ones fail).  The
comment beside each test quotes the dispatch condition that sends its shape to the kernel form it names.

Function constants (fp32_contract.RSQRT_ULPS, EXPF_ULPS, FAST_EXP_ULPS, FAST_LOG_ULPS, RCP_ULPS): each test
that evaluates a device function also prints a `[function]` line: the largest error against the fp64
reference, the structural part of the bound (the bound with the function's constant at 0) subtracted, in
ulp of the function's result.  The rule for the constants is beside them in fp32_contract.py.
"""
import pytest
import torch

import exact as X
import fp32_contract as C

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _ext():
    from naive_gpt import ext as E
    return E


def _cuda(t):
    return None if t is None else t.to(DEV)


def _function_line(name, got, ref, structural, unit):
    """Largest (|got - ref| - structural) / unit: the error left for the function itself, in its ulp."""
    err = (got.detach().double().cpu() - ref).abs() - structural
    live = unit > 0
    worst = float((err[live] / unit[live]).max()) if bool(live.any()) else 0.0
    print('[function] {}: {:.2f} ulp beyond the structural bound'.format(name, worst))
    return worst


# ----------------------------------------------------------------------------------- norm kernels
# spt_layernorm_form(d, rms): d / 256 in {1, 2, 3, 4, 8} -> a wave per row with NV = d / 256 float4 per
# lane; RMS 4096 -> NV 16, gamma re-read per row (GREG = NV <= 8 is false); 2560 -> two waves per row;
# LayerNorm 4096 and 5120 -> four.  The grid is min(ceil(rows / 8), 512) workgroups: at 4096 + 37 rows a
# wave (group) walks more than one row and the wide kernels' exchange slots alternate.
NORM_CASES = [(d, rms, 37, add) for d in (256, 768, 2048, 2560, 4096, 5120) for rms in (False, True)
              for add in (True, False)]
NORM_CASES += [(d, rms, 4096 + 37, True) for d in (768, 5120) for rms in (False, True)]


@pytest.mark.parametrize('d,rms,rows,add', NORM_CASES)
def test_norm_kernels_within_their_bounds(d, rms, rows, add):
    E = _ext()
    assert E.layernorm_form(d, rms) == C.norm_form(d, rms)[1]
    assert E.load_library().spt_layernorm_partial_rows(rows) == C.norm_partial_rows(rows)
    inp = C.norm_inputs(d, rows, rms, seed=d + rows + rms, add=add)
    assert C.small_share(inp['x']) >= 0.1 and C.small_share(inp['dy']) >= 0.1
    s, y, mean, rstd = E.add_layernorm_forward(_cuda(inp['x']), _cuda(inp['r']), _cuda(inp['gamma']),
                                               _cuda(inp['beta']), inp['eps'], rms=rms)
    refs = C.norm_forward_refs(inp, rms)
    what = '{} d={} rows={}{}'.format('rms' if rms else 'ln', d, rows, ' +r' if add else '')
    C.check(dict(s=s, y=y, mean=mean, rstd=rstd), refs, what)
    ref0, bound0 = C.norm_forward_refs(inp, rms, rsqrt=0, only_rstd=True)['rstd']
    _function_line('rsqrtf ' + what, rstd, ref0, bound0, C.U * ref0)
    # the backward on what the forward stored, as autograd hands it over
    dx, dgamma, dbeta = E.layernorm_backward(s, _cuda(inp['dy']), _cuda(inp['gamma']), mean, rstd,
                                             _cuda(inp['dskip']), rms=rms)
    refs = C.norm_backward_refs(inp, s.cpu(), mean.cpu(), rstd.cpu(), rms)
    C.check(dict(dx=dx, dgamma=dgamma, dbeta=dbeta), refs, what)


# -------------------------------------------------------------------------------------- head loss
# spt_cross_entropy_grad: `ld <= 4 * HL_THREADS * HL_MAXJ` (32768) -> the resident form (the row in
# registers); above -> the streaming form (the row read three times).
@pytest.mark.parametrize('V,ld', [(1001, 1008), (32768 + 8, 32768 + 8)])
def test_head_loss_within_its_bound(V, ld):
    E = _ext()
    inp = C.head_loss_inputs(V, ld, seed=V)
    refs = C.head_loss_refs(inp)
    assert C.small_share(refs['grad'][0]) >= 0.1
    logits = inp['logits'].to(DEV)
    loss = E.cross_entropy_grad_(logits, V, inp['target'].to(DEV), inp['scale'].to(DEV))
    C.check(dict(loss=loss, grad=logits), refs, 'head loss V={}'.format(V))
    ref0 = C.head_loss_refs(inp, fast_exp=0, fast_log=0)
    _function_line('__expf (gradient) V={}'.format(V), logits, ref0['grad'][0], ref0['grad'][1],
                   C.U * (ref0['grad'][0] + torch.zeros_like(ref0['grad'][0]).scatter_(
                       1, inp['target'].clamp_min(0)[:, None], inp['scale'].double().item())).abs())
    _function_line('__logf (loss) V={}'.format(V), loss, ref0['loss'][0], ref0['loss'][1],
                   C.U * (ref0['loss'][0] != 0).double())


# ---------------------------------------------------------------------------------- sparse softmax
# softmax_launch: G = pow2_ceil((nnz / S + 3) / 4), at least 4: Z = 16 -> G = 4, Z = 64 -> G = 16; the
# float4 path needs `((start | end | nnz) & 3) == 0`, so the ragged pattern takes the scalar path.
@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('kind', ['z16', 'z64', 'ragged'])
def test_softmax_within_its_bounds(kind, causal):
    E = _ext()
    inp = C.softmax_inputs(kind, causal, seed=len(kind) + causal)
    if kind != 'ragged':
        assert C.softmax_group(inp['nnz'], inp['S']) == {'z16': 4, 'z64': 16}[kind]
    else:
        assert (inp['indptr'][:-1] % 4 != 0).any()
    refs = C.softmax_forward_refs(inp)
    assert C.small_share(refs['y'][0]) >= 0.1
    floored = C._row_sums(refs['y'][0], inp['row_of'], inp['S']) < 0.5
    assert floored.any()                                              # rows under the 1e-9 floor
    indptr, indices = inp['indptr'].to(DEV), inp['indices'].to(DEV)
    y = E.softmax_forward_cuda(indptr, indices, inp['values'].to(DEV))
    what = 'softmax {} causal={}'.format(kind, causal)
    C.check(dict(y=y), refs, what)
    ref0 = C.softmax_forward_refs(inp, expf=0)['y']
    _function_line('expf ' + what, y, ref0[0], ref0[1], C.U * ref0[0])
    grad = E.softmax_backward_cuda(indptr, indices, y, inp['dy'].to(DEV))
    C.check(dict(grad=grad), C.softmax_backward_refs(inp, y.cpu()), what + ' backward')
    scores = C.softmax_clamped_scores(inp)
    assert (scores.abs() == inp['clamp']).float().mean() > 0.2
    grad = E.softmax_backward_clamped(indptr, indices, y, inp['dy'].to(DEV), scores.to(DEV), inp['scale'],
                                      inp['clamp'])
    C.check(dict(grad=grad), C.softmax_backward_refs(inp, y.cpu(), clamped=scores), what + ' backward, clamped')


# ------------------------------------------------------------------------------------ elementwise
# T = 1000 rows: spt_swiglu_backward launches (rows + 3) / 4 workgroups of four waves, a wave per row;
# n = 520 is 2 steps of 256 columns and a partial third.
def test_swiglu_within_its_bounds():
    E = _ext()
    inp = C.swiglu_inputs(1000, 520, seed=3)
    g, s, dh = (inp[k].to(DEV) for k in ('g', 's', 'dh'))
    refs = C.swiglu_forward_refs(inp)
    assert C.small_share(refs['h'][0]) >= 0.1
    h = E.swiglu_forward(g, s)
    C.check(dict(h=h), refs, 'swiglu_forward')
    ref0 = C.swiglu_forward_refs(inp, expf=0)['h']
    _function_line('expf (silu)', h, ref0[0], ref0[1], C.U * ref0[0].abs())
    dg, ds, dot_h, dot_g, dot_s = E.swiglu_backward(dh, g, s)
    C.check(dict(dg=dg, ds=ds, dot_h=dot_h, dot_g=dot_g, dot_s=dot_s), C.swiglu_backward_refs(inp, dg, ds),
            'swiglu_backward')


@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('n_parts,n_rot', [(1, 1), (2, 2), (3, 2), (2, 0)])
def test_rotary_within_its_bound(n_parts, n_rot, transpose):
    E = _ext()
    inp = C.rotary_inputs(n_parts, seed=n_parts + n_rot)
    assert C.small_share(torch.stack(inp['parts'])) >= 0.1
    out = E.rotary([p.to(DEV) for p in inp['parts']], n_rot, inp['cos'].to(DEV), inp['sin'].to(DEV),
                   transpose=transpose)
    C.check(dict(out=out), C.rotary_refs(inp, n_rot, transpose),
            'rotary parts={} n_rot={} transpose={}'.format(n_parts, n_rot, transpose))


# T = 1000: four chunks of 256 tokens, the last one partial (route_topk_kernel counts through all of them).
@pytest.mark.parametrize('G,k', [(4, 2), (8, 2), (6, 3)])
def test_routing_passes_within_their_bounds(G, k):
    E = _ext()
    T = 1000
    inp = C.route_inputs(T, G, seed=G + k)
    inp['dcoeff'] = inp['dcoeff'].repeat(2)[:T * k].contiguous()
    assert C.small_share(inp['prob']) >= 0.1
    # coeff = fl(scale prob): one rounding
    token, block, pos = C.route_selection(inp['prob'].double(), k)
    got = E.route_topk_coeff(inp['prob'].to(DEV), k, inp['scale'])
    assert torch.equal(got[0].cpu().long(), token) and torch.equal(got[1].cpu().long(), block)
    assert torch.equal(got[3].cpu().long(), pos)
    want = inp['scale'] * inp['prob'].double()[token, block]
    X.assert_within(got[6], want, C.U * want.abs(), 'route_topk_coeff G={} k={}'.format(G, k))
    # from the logits: the probabilities, and the coefficients from the STORED probabilities
    prob_ref, prob_bound = C.route_prob_refs(inp)
    token, block, pos = C.route_selection(inp['logits'][:, :G].double() + inp['bias'].double(), k)
    got = E.route_topk_logits(inp['logits'].to(DEV)[:, :G], inp['bias'].to(DEV), G, k, inp['scale'])
    assert torch.equal(got[1].cpu().long(), token) and torch.equal(got[2].cpu().long(), block)
    assert torch.equal(got[4].cpu().long(), pos)
    X.assert_within(got[0], prob_ref, prob_bound, 'route_topk_logits prob G={} k={}'.format(G, k))
    want = inp['scale'] * got[0].double().cpu()[token, block]
    X.assert_within(got[7], want, C.U * want.abs(), 'route_topk_logits coeff G={} k={}'.format(G, k))
    ref0 = C.route_prob_refs(inp, expf=0)
    _function_line('expf (router sigmoid)', got[0], ref0[0], ref0[1], C.U * ref0[0])
    for prob in (None, got[0]):
        out = E.route_coeff_backward(inp['dcoeff'].to(DEV), got[4], got[2], inp['scale'], G, prob=prob)
        refs = C.route_backward_refs(inp, token, block, None if prob is None else prob.cpu())
        name = next(iter(refs))
        C.check({name: out}, refs, 'route_coeff_backward G={} k={}'.format(G, k))


def test_ffn_coeff_grad_within_its_bound():
    E = _ext()
    inp = C.ffn_coeff_inputs(1000, 500, 6, 16, seed=2)
    assert (inp['coeff'] < inp['floor']).any() and (inp['coeff'] > inp['floor']).any()
    out = E.ffn_coeff_grad(*(inp[n].to(DEV) for n in ('dot_main', 'dot_act', 'du', 'u', 'dzt', 'z', 'token', 'coeff')),
                           inp['floor'])
    refs = C.ffn_coeff_refs(inp)
    assert C.small_share(refs['out'][0]) >= 0.1
    C.check(dict(out=out), refs, 'ffn_coeff_grad')


def test_embedding_rows_backward_within_its_bound():
    E = _ext()
    inp = C.embedding_inputs(4096, 16, 5000, seed=3)
    assert int((inp['ids'] == 0).sum()) == 3000 and inp['ids'].unique().numel() == 4096 - 3000 + 1
    out = E.embedding_rows_backward(inp['grad'].to(DEV), inp['ids'].to(DEV), inp['n_rows'])
    C.check(dict(out=out), C.embedding_refs(inp), 'embedding_rows_backward')


@pytest.mark.parametrize('with_side', [False, True])
def test_rows_combine_within_its_bound(with_side):
    E = _ext()
    inp = C.combine_inputs(1000, 2, 24, 4, seed=4)
    kw = dict(side=inp['side'].to(DEV), side_weight=inp['side_weight'].to(DEV)) if with_side else {}
    out = E.rows_combine(inp['rows'].to(DEV), inp['pos'].to(DEV), inp['bias'].to(DEV), **kw)
    C.check(dict(out=out), C.combine_refs(inp, with_side), 'rows_combine side={}'.format(with_side))


# ------------------------------------------------------------------- sddmm / spmm, gather forms
# spt_sddmm_forward with SPT_SDDMM_GATHER=1 (the tile form refuses): E = 64 / 128 -> sddmm_g4_launch:
# `kbytes <= 128 KiB && B * 8 >= 256` -> sddmm_g4_lds, else sddmm_g4_global; other E:
# `kbytes <= 128 KiB && B * 8 >= 256 && S >= 64` -> sddmm_lds, else sddmm_global.
SDDMM_CASES = [(32, 96, 20, 'z16', 'sddmm_lds'), (3, 96, 20, 'ragged', 'sddmm_global'),
               (32, 96, 64, 'z16', 'sddmm_g4_lds'), (32, 96, 128, 'ragged', 'sddmm_g4_lds, 8 lanes per entry'),
               (3, 96, 64, 'ragged', 'sddmm_g4_global'), (3, 96, 128, 'z16', 'sddmm_g4_global, 8 lanes per entry')]


@pytest.mark.parametrize('B,S,E,kind,form', SDDMM_CASES)
def test_sddmm_gather_forms_within_their_bound(B, S, E, kind, form, monkeypatch):
    Ex = _ext()
    monkeypatch.setenv('SPT_SDDMM_GATHER', '1')                      # (read by the library at every call)
    inp = C.sparse_inputs(B, S, E, kind, seed=B + E)
    assert C.small_share(inp['q']) >= 0.1
    f, t = torch.scalar_tensor(False), torch.scalar_tensor(True)
    for scale, clamp in ((1.0, 0.0), (E ** -0.5 * 4, 10.0)):
        refs = C.sddmm_refs(inp, scale, clamp)
        assert clamp == 0 or (refs['out'][0].abs() == clamp).any()
        Ex.reset_paths()
        out = Ex.sddmm_forward_cuda(f, t, inp['indptr'].to(DEV), inp['indices'].to(DEV), inp['q'].to(DEV),
                                    inp['k'].to(DEV), scale=scale, clamp=clamp)
        assert Ex.paths_taken('sddmm') == {('sddmm', 'gather'): 1}
        C.check(dict(out=out), refs, '{} scale={:.2f} clamp={}'.format(form, scale, clamp))


# launch_gather of spmm.hip: transposed && E == 64 && tile <= 128 KiB && B >= 128 -> spmm_t64_lds; E = 64 /
# 128: `tile_bytes <= 128 KiB && B >= 32` -> spmm_g4_lds, else spmm_g4_global; other E -> spmm_generic.
# chunked_layout: `E == 64 && S > 512 && S % 512 == 0` -> the chunked transposed form.
SPMM_CASES = [(3, 96, 20, 'z16', 'spmm_generic'), (32, 96, 64, 'ragged', 'spmm_g4_lds'),
              (3, 96, 128, 'z16', 'spmm_g4_global'), (128, 64, 64, 'z16', 'spmm_t64_lds (T)'),
              (2, 1024, 64, 'z16', 'chunked (T)')]


@pytest.mark.parametrize('B,S,E,kind,form', SPMM_CASES)
def test_spmm_gather_forms_within_their_bound(B, S, E, kind, form):
    Ex = _ext()
    inp = C.sparse_inputs(B, S, E, kind, seed=B + E + 1)
    assert C.small_share(inp['values']) >= 0.1
    f = torch.scalar_tensor(False)
    indptr, indices, values, x = (inp[n].to(DEV) for n in ('indptr', 'indices', 'values', 'x'))
    Ex.reset_paths()
    y = Ex.spmm_forward_cuda(f, f, indptr, indices, values, x)
    assert Ex.paths_taken('spmm') == {('spmm', 'gather'): 1}
    C.check(dict(y=y), C.spmm_refs(inp, False), form + ' N')
    refs = C.spmm_refs(inp, True)
    y = Ex.spmm_forward_cuda(torch.scalar_tensor(True), f, indptr, indices, values, x)
    C.check(dict(y=y), refs, form + ' T')
    y = Ex.spmm_transposed(Ex.csr_transpose(indptr, indices, E), indptr, indices, values, x)
    C.check(dict(y=y), refs, form + ' csr_transpose + spmm_transposed')
    y = Ex.spmm_transposed(Ex.transposed_for(indptr, indices, E), indptr, indices, values, x)       # the memo in front
    C.check(dict(y=y), refs, form + ' transposed_for + spmm_transposed')


# ------------------------------------------------------------------------------ fused attention
# fused_attention_supported: E == 64, Z <= 64, Z % 4 == 0, S E 4 <= 128 KiB, B >= 32.  Z = 16: one entry
# group of a row's four holds entries; Z = 64: all four.
@pytest.mark.parametrize('yt', [False, True])
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('Z', [16, 64])
def test_fused_attention_within_the_chain_bound(Z, causal, yt):
    E = _ext()
    N, H, S = 2, 16, 256
    inp = C.attention_inputs(N, H, S, Z, causal, seed=Z + causal)
    assert E.fused_attention_supported(S, 64, N * H, S * Z)
    refs = C.attention_forward_refs(inp)
    assert (refs['scores'][0].abs() == inp['clamp']).any() and C.small_share(refs['y'][0]) >= 0.1
    indices = inp['indices'].to(DEV)
    q, k, v = (inp[n].to(DEV) for n in ('q', 'k', 'v'))
    scores, attn, y = E.sparse_attention_forward(indices, q, k, v, inp['scale'], inp['clamp'], y_transposed=yt,
                                                 causal=causal)
    what = 'fused attention Z={} causal={} yt={}'.format(Z, causal, yt)
    C.check(dict(scores=scores, attn=attn, y=y.transpose(1, 2) if yt else y), refs, what)
    ref0 = C.attention_forward_refs(inp, expf=0)['attn']
    _function_line('expf ' + what, attn, ref0[0], ref0[1], C.U * ref0[0])
    # the backward on the scores / attn the forward stored, dy in the layout autograd hands back
    dy = inp['dy'].transpose(1, 2).contiguous() if yt else inp['dy']
    grad_raw, grad_q, rows = E.sparse_attention_backward_rows(indices, dy.to(DEV), v, k, scores, attn, inp['scale'],
                                                              inp['clamp'], grad_y_transposed=yt, causal=causal)
    assert torch.equal(rows.cpu(), inp['dy'])
    brefs = C.attention_backward_refs(inp, scores.cpu(), attn.cpu())
    assert (brefs['grad_raw'][0] == 0).any()
    C.check(dict(grad_raw=grad_raw, grad_q=grad_q), brefs, what + ' backward')


# ------------------------------------------------------------------------------------------- PQ
# M D = 64 and 80 (M = 8: a power of two, the lanes of a wave that share a subspace merge by butterfly; M = 10:
# by ascending additions), C = 16, 2 x 256 x 4 head vectors per part; the pair forms take q and k back to back.
@pytest.mark.parametrize('M', [8, 10])
def test_pq_loss_within_its_bounds(M):
    E = _ext()
    inp = C.pq_inputs(M, seed=M)
    assert C.small_share(inp['z']) >= 0.1
    refs = C.pq_refs(inp)
    z, table, gl = inp['z'][0].to(DEV), inp['table'].to(DEV), inp['grad_loss'].to(DEV)
    loss = E.pq_loss_forward(z, table)
    grad_z, grad_w = E.pq_loss_backward(z, table, gl)
    C.check(dict(loss=loss, grad_z=grad_z[None], grad_weight=grad_w), refs, 'pq_loss M={}'.format(M))
    # the pair forms: loss_q + loss_k, the gradients ADDED into what grad_q / grad_k already hold
    inp = C.pq_inputs(M, seed=M + 1, parts=2)
    refs = C.pq_refs(inp, accumulate=True)
    pair, grads = inp['z'].to(DEV), inp['prior'].to(DEV)
    table = inp['table'].to(DEV)
    loss, _, _ = E.pq_loss_forward_pair(pair[0], pair[1], table)
    grad_w = E.pq_loss_backward_pair(pair[0], pair[1], table, gl, grads[0], grads[1])
    C.check(dict(loss=loss, grad_z=grads, grad_weight=grad_w), refs, 'pq_loss pair M={}'.format(M))


@pytest.mark.parametrize('M', [8, 10])
def test_cdist_backward_within_its_bound(M):
    E = _ext()
    inp = C.pq_inputs(M, seed=M + 2)
    D = inp['table'].size(-1)
    query = inp['z'].view(-1, M, D).transpose(0, 1).contiguous()              # [M, NQ, D]; some rows ARE codewords
    gen = torch.Generator().manual_seed(M)
    go = torch.randn([M, query.size(1), 16], generator=gen) * torch.pow(2.0, -C.row_exponents(query.size(1)).float())[:, None]
    assert (query[:, :, None, :] == inp['table'][:, None, :, :]).any()
    gq, gt = E.cdist_backward_cuda(query.to(DEV), inp['table'].to(DEV), go.to(DEV))
    C.check(dict(grad_query=gq, grad_table=gt), C.cdist_backward_refs(query, inp['table'], go), 'cdist_backward M={}'.format(M))
