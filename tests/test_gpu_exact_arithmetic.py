"""GPU tier, exact: the matrix-core kernels on inputs they must reproduce bit for bit (tests/exact.py).

Integer operands, one of every product with at most 16 significant bits (hi + lo == x) and the other
exact in bf16, every partial sum below 2^24: the split-bf16 fp32 path then has no error at all, in any
order and at any MFMA shape, and every assertion here is `torch.equal` against an fp64 reference
(exact on these inputs).  bf16-storing kernels must store `rne_bf16` of the exact fp32 result: ties
included, no band.  The two-part values sit in one operand per case and in the other in its twin, so
each of the split's cross terms (hi.lo, lo.hi) is pinned on its own.  Where a case depends on a
dispatch condition the test asserts it (`ext.LAST_GEMM_PATH`, `ext.paths_taken`, the form queries).
"""
import pytest
import torch

import exact as X

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _offsets(sizes):
    cuts = [0]
    for s in sizes:
        cuts.append(cuts[-1] + s)
    return cuts


def _operands(gen, two_part, shape_a, shape_w, k, extra):
    """(a, w) fp32 on the host: the two-part values in `two_part` ('a' / 'w'), bf16 integers in the other,
    sized from k so that every sum (plus `extra`) stays exact."""
    # the main sum gets 2^21 (less `extra`): times a rowscale of 2 at most, in units of 1/2, below 2^24
    other = max(1, min(64, int(2 ** 21 / ((1 + 2 ** -7) * k * 2048))))
    bound = X.two_part_bound(k, other, extra=X.EXACT_LIMIT - 2 ** 21 + extra)
    if two_part == 'a':
        return X.two_part_ints(gen, shape_a, bound), X.bf16_ints(gen, shape_w, other)
    return X.bf16_ints(gen, shape_a, other), X.two_part_ints(gen, shape_w, bound)


def _ref(a_rows, wg_list, sizes, bias=None, rowscale=None, side=None, acc=None):
    """fp64 [P, N]: rows of group g = a_rows[g] @ W_g^T (+ bias[g]), times rowscale, + side, + acc."""
    outs = []
    for g, s in enumerate(sizes):
        o = a_rows[g].double() @ wg_list[g].double().T
        if bias is not None:
            o = o + bias[g].double()
        outs.append(o)
    out = torch.cat(outs) if outs else None
    if rowscale is not None:
        out = out * rowscale.double()[:, None]
    if side is not None:
        out = out + side
    if acc is not None:
        out = out + acc.double()
    return out


def _check(got, want, what):
    got = got.double().cpu()
    want = want.cpu()
    if not torch.equal(got, want):
        bad = (got != want)
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError('{}: {} of {} elements differ (first at {}: got {}, exact {})'.format(
            what, int(bad.sum()), bad.numel(), i, got.reshape(-1)[i].item(), want.reshape(-1)[i].item()))


# ---------------------------------------------------------------------------------- grouped_gemm (fp32)

# name, K, N, sizes, layout, path, extras
FUSED = [
    ('reg_ktail', 100, 200, [0, 129, 1, 0, 127, 128, 0], 'bt', 'register', {}),
    ('reg_k32', 96, 160, [0, 129, 1, 0, 127, 128, 0], 'bt', 'register', {}),
    ('reg_bn_ktail', 68, 96, [1, 0, 300, 129], 'bn', 'register', {}),
    ('img_bt', 128, 192, [0, 129, 1, 0, 127, 128, 0], 'bt', 'image', {}),
    ('img_bn', 96, 128, [1, 0, 300, 129], 'bn', 'image', {}),
    ('a32_bt', 128, 200, [0, 129, 1, 0, 127, 128, 0], 'bt', 'a32', {}),
    ('a32_bn', 64, 96, [128, 0, 129, 1], 'bn', 'a32', {}),
    ('ext_r32_reg', 64, 130, [0, 200, 1, 129, 0], 'bt', 'register', {'r': 32}),
    ('ext_r16_img', 64, 128, [0, 200, 1, 129, 0], 'bt', 'image', {'r': 16}),
    ('ext_r8_a32_bn', 64, 128, [3, 0, 250], 'bn', 'a32', {'r': 8}),
    ('ext_r48_b2seg', 64, 128, [0, 200, 1, 129, 0], 'bt', 'register', {'r': 48, 'b2_seg': True}),
    ('ext_r64_b2seg', 96, 96, [131, 0, 127], 'bt', 'register', {'r': 64, 'b2_seg': True}),
    ('a_seg', 96, 128, [0, 129, 1, 0, 300], 'bt', 'register', {'a_seg': 32}),
    ('accumulate_ldo', 64, 100, [0, 129, 1, 127, 0], 'bt', 'register', {'accumulate': True, 'ldo': 112}),
    ('accumulate_img', 64, 128, [0, 129, 1, 127, 0], 'bt', 'image', {'accumulate': True, 'ldo': 160}),
]


def _fused_case(name, K, N, sizes, layout, path, extras, two_part, seed):
    gen = _gen(seed)
    G, P = len(sizes), sum(sizes)
    r = extras.get('r', 0)
    T = P + 37
    extra = 2 ** 12 + (2 ** 17 if r else 0) + (2 ** 11 if extras.get('accumulate') else 0)
    a, w_nk = _operands(gen, two_part, [T, K], [G, N, K], K, extra)
    gather = torch.randint(0, T, [P], generator=gen, dtype=torch.int32)
    bias = X.bf16_ints(gen, [G, N], 64)
    rowscale = X.pow2_rowscale(gen, P, -1, 1)
    rows = [a[gather[lo:hi].long()] for lo, hi in zip(_offsets(sizes)[:-1], _offsets(sizes)[1:])]
    side = None
    kw = {}
    if layout == 'bt':
        w = w_nk.reshape(G * N, K)
        view = (N * K, K, 1)
    else:
        w = w_nk.permute(2, 0, 1).reshape(K, G * N).contiguous()      # W_g(n, k) = w[k, g N + n]
        view = (N, 1, G * N)
    if r:
        T2 = P + 5
        # the side product's two-part values in the other operand than the main product's: |side| < 2^17
        if two_part == 'a':
            a2, b2 = X.bf16_ints(gen, [T2, r], 1), X.two_part_ints(gen, [G, N, r], 2047)
        else:
            a2, b2 = X.two_part_ints(gen, [T2, r], 2047), X.bf16_ints(gen, [G, N, r], 1)
        gather2 = torch.randint(0, T2, [P], generator=gen, dtype=torch.int32)
        side = torch.cat([a2[gather2[lo:hi].long()].double() @ b2[g].double().T
                          for g, (lo, hi) in enumerate(zip(_offsets(sizes)[:-1], _offsets(sizes)[1:]))])
        X.fits_fp32(2 ** 22 + 2 ** 12 + float(side.abs().max()), 1 / 2)     # rowscale <= 2: main + bias <= 2^22
        if extras.get('b2_seg'):
            seg = G * N * 16 + 64                          # tables lie that many floats apart
            flat = torch.zeros([r // 16 * seg], dtype=torch.float32)
            for j in range(r // 16):
                flat[j * seg:j * seg + G * N * 16] = b2[:, :, 16 * j:16 * j + 16].reshape(-1)
            flat = flat.to(DEV)
            kw.update(b2=flat[:G * N * 16].view(G, N, 16), b2_group_stride=N * 16, b2_segment_stride=seg,
                      keep=flat)
        else:
            kw.update(b2=b2.to(DEV), b2_group_stride=N * r)
        kw.update(a2=a2.to(DEV), gather2=gather2.to(DEV))
    want = _ref(rows, list(w_nk), sizes, bias, rowscale, side)
    a_dev = a.to(DEV)
    if extras.get('a_seg'):
        seg_k = extras['a_seg']
        stride = T * seg_k + 96
        flat = torch.zeros([K // seg_k * stride], dtype=torch.float32)
        for j in range(K // seg_k):
            flat[j * stride:j * stride + T * seg_k] = a[:, j * seg_k:(j + 1) * seg_k].reshape(-1)
        flat = flat.to(DEV)
        a_dev = flat[:T * seg_k].view(T, seg_k)
        kw.update(a_segments=(seg_k, stride), keep_a=flat)
    if path in ('image', 'a32'):
        kw['w_image'] = ext().split_bf16(w.to(DEV))
        if path == 'image':
            kw['a_image'] = ext().split_bf16(a_dev)
    if extras.get('accumulate'):             # out: [P, N] of a [P, ldo] buffer, the padding left alone
        base = X.bf16_ints(gen, [P, extras['ldo']], 256) * 4
        buf = base.to(DEV)
        want = want + base[:, :N].double()
        kw.update(out=buf[:, :N], accumulate=True, _base=base, keep=buf)
    return dict(a=a_dev, w=w.to(DEV), sizes=sizes, G=G, N=N, K=K, P=P, view=view, gather=gather.to(DEV),
                bias=bias.to(DEV), rowscale=rowscale.to(DEV), want=want, kw=kw, path=path)


def ext():
    from naive_gpt import ext as E
    return E


def _run_fused(c, **more):
    E = ext()
    kw = {k: v for k, v in c['kw'].items() if k not in ('keep', 'keep_a', '_base')}
    kw.update(more)
    offsets = torch.tensor(_offsets(c['sizes']), dtype=torch.int32, device=DEV)
    out = E.grouped_gemm_fused(c['a'], c['w'], offsets, c['G'], c['N'], c['K'], *c['view'], c['P'],
                               gather=c['gather'], bias=c['bias'], rowscale=c['rowscale'], **kw)
    return out


@pytest.mark.parametrize('two_part', ['a', 'w'])
@pytest.mark.parametrize('case', FUSED, ids=[f[0] for f in FUSED])
def test_grouped_gemm_fused_is_exact(case, two_part):
    name, K, N, sizes, layout, path, extras = case
    c = _fused_case(name, K, N, sizes, layout, path, extras, two_part, seed=sum(map(ord, name)) + (two_part == 'w'))
    E = ext()
    out = _run_fused(c)
    assert E.LAST_GEMM_PATH == path, (name, E.LAST_GEMM_PATH)
    assert path != 'register' or (K % 32 != 0) == name.endswith('ktail')       # the k-tail kernel or not
    _check(out, c['want'], name)
    if extras.get('accumulate'):
        assert out.stride(0) == extras['ldo']
        _check(c['kw']['keep'][:, N:], c['kw']['_base'][:, N:].double(), name + ': the padding past n')


@pytest.mark.parametrize('form', ['image', 'a32'])
def test_ring_form_is_exact(form, monkeypatch):
    """SPT_GEMM_RING=1 (read at every call): the loader / consumer form of the plain image-path GEMM.
    The library also needs the resident workgroup count to be a multiple of 16 (launch_grouped), true of
    the MI355X's 256 CUs x 2; that condition is assumed here, not observed: LAST_GEMM_PATH reads 'image' /
    'a32' with or without the ring."""
    monkeypatch.setenv('SPT_GEMM_RING', '1')
    for two_part in ('a', 'w'):
        for r in (0, 16):
            c = _fused_case('ring', 128, 256, [0, 700, 1, 129, 0, 300], 'bt', form, {'r': r} if r else {},
                            two_part, seed=7 + r)
            out = _run_fused(c)
            assert ext().LAST_GEMM_PATH == form
            _check(out, c['want'], 'ring {} {} r={}'.format(form, two_part, r))


def test_plain_grouped_gemm_is_exact():
    """spt_grouped_gemm: both orientations, K tail, gather, bias, rowscale."""
    E = ext()
    for layout, K in (('bt', 100), ('bn', 64), ('bt', 256)):
        for two_part in ('a', 'w'):
            c = _fused_case('plain', K, 96, [0, 129, 1, 0, 127, 128, 0], layout, 'register', {}, two_part, seed=K)
            offsets = torch.tensor(_offsets(c['sizes']), dtype=torch.int32, device=DEV)
            out = E.grouped_gemm(c['a'], c['w'], offsets, c['G'], c['N'], c['K'], *c['view'],
                                 gather=c['gather'], bias=c['bias'], rowscale=c['rowscale'])
            _check(out, c['want'], 'grouped_gemm {} K={} {}'.format(layout, K, two_part))


# ------------------------------------------------------------------------- ReLU at an exact zero

@pytest.mark.parametrize('G', [5, 260])
@pytest.mark.parametrize('path', ['register', 'image'])
def test_relu_at_exact_zero_pre_activations(G, path):
    """Small integers make many pre-activations exactly 0: ACT gives 0 there, the DACT mask is torch's
    (x > 0: the derivative at 0 is 0), and the DACT row dots equal the integer reference.  G = 5 and
    G = 260 lie on either side of the library's rule for the near-the-kink queue (launch_grouped: G < 256
    queues the elements for relu_fix_kernel, otherwise the epilogue recomputes them itself); which one
    ran is not visible from here, so both are held to the same exact result."""
    E = ext()
    gen = _gen(G + len(path))
    K, N = 64, 128
    sizes = [0] * G
    sizes[1], sizes[G // 2], sizes[-2] = 129, 1, 200
    P = sum(sizes)
    a = torch.randint(-1, 2, [P, K], generator=gen).float()
    w = torch.randint(-1, 2, [G * N, K], generator=gen).float()
    w[:, ::3] = 0
    bias = torch.randint(-1, 2, [G, N], generator=gen).float()
    offsets = torch.tensor(_offsets(sizes), dtype=torch.int32, device=DEV)
    rows = [a[lo:hi] for lo, hi in zip(_offsets(sizes)[:-1], _offsets(sizes)[1:])]
    pre = _ref(rows, list(w.view(G, N, K)), sizes, bias)
    zeros = int((pre == 0).sum())
    assert zeros > 0.05 * pre.numel()
    kw = {}
    if path == 'image':
        kw = dict(a_image=E.split_bf16(a.to(DEV)), w_image=E.split_bf16(w.to(DEV)))
    h, kept = E.grouped_gemm_fused(a.to(DEV), w.to(DEV), offsets, G, N, K, N * K, K, 1, P, bias=bias.to(DEV),
                                   epilogue=E.EPI_ACT, activation=E.ACT_RELU, keep_preact=True, **kw)
    assert E.LAST_GEMM_PATH == path
    _check(kept, pre, 'ReLU pre-activation')
    _check(h, pre.clamp_min(0), 'ReLU output')
    # DACT: v = dY W2^T (here: the same product), mask from h_in = relu(s) (s_in NULL) and from s_in
    dy = a
    v = pre
    s = X.bf16_ints(gen, [P, N], 3)
    s[:, ::4] = 0
    hs = s.clamp_min(0)
    for s_in in (None, s):
        kw_d = dict(s_in=s_in.to(DEV)) if s_in is not None else dict(h_in=hs.to(DEV))
        out, dm, da = E.grouped_gemm_fused(dy.to(DEV), w.to(DEV), offsets, G, N, K, N * K, K, 1, P,
                                           bias=bias.to(DEV), epilogue=E.EPI_DACT, activation=E.ACT_RELU,
                                           **kw, **kw_d)
        want = v * (s > 0).double()
        _check(out, want, 'DACT ReLU output (s_in {})'.format(s_in is not None))
        _check(dm, (v * hs.double()).sum(1), 'pdot_main')
        _check(da, (want * s.double()).sum(1), 'pdot_act')


# ------------------------------------------------------------------------------ weight gradients

@pytest.mark.parametrize('bf16', [False, True])
def test_grouped_gemm_wgrad_is_exact(bf16):
    """dW_g = sum_p rowscale[p] G[srcG(p)] (x) A[srcA(p)], dbias likewise: gather on either operand,
    empty groups and a group of more than one 512-row chunk."""
    E = ext()
    gen = _gen(11 + bf16)
    n, k = 96, 128
    sizes = [0, 1100, 1, 0, 129, 300, 0]
    G, P = len(sizes), sum(sizes)
    offsets = torch.tensor(_offsets(sizes), dtype=torch.int32, device=DEV)
    for gather_on in ('g', 'a'):
        T = P + 11
        if bf16:
            g_op = X.bf16_ints(gen, [T, n], 4)
            a_op = X.bf16_ints(gen, [T, k], 4)
        else:
            g_op, a_op = _operands(gen, 'a' if gather_on == 'g' else 'w', [T, n], [T, k], 1100, 0)
        gather = torch.randint(0, T, [P], generator=gen, dtype=torch.int32)
        rowscale = X.pow2_rowscale(gen, P, -1, 1)
        src = gather.long()
        rows = torch.arange(P)
        gsrc, asrc = (src, rows) if gather_on == 'g' else (rows, src)
        dt = torch.bfloat16 if bf16 else torch.float32
        out, dbias = E.grouped_gemm_wgrad(
            g_op.to(dt).to(DEV), a_op.to(dt).to(DEV), offsets, (n, k, n * k, k, 1), P,
            gather_grad=gather.to(DEV) if gather_on == 'g' else None,
            gather_a=gather.to(DEV) if gather_on == 'a' else None, rowscale=rowscale.to(DEV), want_bias=True)
        want = torch.zeros([G, n, k], dtype=torch.float64)
        wantb = torch.zeros([G, n], dtype=torch.float64)
        for gi, (lo, hi) in enumerate(zip(_offsets(sizes)[:-1], _offsets(sizes)[1:])):
            gg = g_op[gsrc[lo:hi]].double() * rowscale[lo:hi, None].double()
            want[gi] = gg.T @ a_op[asrc[lo:hi]].double()
            wantb[gi] = gg.sum(0)
        X.fits_fp32(float(want.abs().max()) * 4, 0.5)
        if bf16:
            X.assert_once_rounded(out.view(G, n, k), want, 0.0, 'wgrad_bf16 gather ' + gather_on)
            X.assert_once_rounded(dbias, wantb, 0.0, 'wgrad_bf16 dbias')
        else:
            _check(out.view(G, n, k), want, 'wgrad gather ' + gather_on)
            _check(dbias, wantb, 'wgrad dbias')


# ------------------------------------------------------------------------- bf16 grouped GEMMs

@pytest.mark.parametrize('layout', ['bt', 'bn'])
@pytest.mark.parametrize('epi', ['plain', 'relu', 'accumulate'])
def test_grouped_gemm_bf16_stores_rne_of_the_exact_sum(layout, epi):
    E = ext()
    gen = _gen(len(layout) * 7 + len(epi))
    K, N = 128, 96
    sizes = [0, 129, 1, 0, 127, 128, 300, 0]
    G, P = len(sizes), sum(sizes)
    T = P + 9
    a = X.bf16_ints(gen, [T, K], 12)
    w_nk = X.bf16_ints(gen, [G, N, K], 12)
    bias = X.bf16_ints(gen, [G, N], 256)
    rowscale = X.pow2_rowscale(gen, P, -2, 1)
    gather = torch.randint(0, T, [P], generator=gen, dtype=torch.int32)
    if layout == 'bt':
        w = w_nk.reshape(G * N, K)
        view = (N * K, K, 1)
    else:
        w = w_nk.permute(2, 0, 1).reshape(K, G * N).contiguous()
        view = (N, 1, G * N)
    rows = [a[gather[lo:hi].long()] for lo, hi in zip(_offsets(sizes)[:-1], _offsets(sizes)[1:])]
    want = _ref(rows, list(w_nk), sizes, bias, rowscale)
    X.fits_fp32(float(want.abs().max()) * 8, 0.25)
    offsets = torch.tensor(_offsets(sizes), dtype=torch.int32, device=DEV)
    bf = lambda t: t.to(torch.bfloat16).to(DEV)
    args = (bf(a), bf(w), offsets, G, N, K) + view
    kw = dict(gather=gather.to(DEV), bias=bf(bias), rowscale=rowscale.to(DEV))
    if epi == 'plain':
        out = E.grouped_gemm_bf16(*args, **kw)
    elif epi == 'relu':
        out, pre = E.grouped_gemm_bf16(*args, **kw, epilogue=E.EPI_ACT, activation=E.ACT_RELU, keep_preact=True)
        X.assert_once_rounded(pre, want, 0.0, 'bf16 pre-activation')
        want = want.clamp_min(0)
    else:
        base = X.bf16_ints(gen, [P, N], 256) * 8
        out = bf(base)
        E.grouped_gemm_bf16(*args, **kw, out=out, accumulate=True)
        want = want + base.double()
    n_ties = int((want.reshape(-1) == X.bf16_brackets(want.reshape(-1))[2]).sum())
    assert n_ties > 0.01 * want.numel(), n_ties          # ties-to-even is exercised
    X.assert_once_rounded(out, want, 0.0, 'grouped_gemm_bf16 ' + epi)


@pytest.mark.parametrize('r', [4, 16, 32])
@pytest.mark.parametrize('epi', ['plain', 'relu', 'accumulate'])
def test_grouped_gemm_bf16_ext_stores_rne_of_the_exact_sum(r, epi):
    E = ext()
    gen = _gen(r * 3 + len(epi))
    K, N = 64, 128
    sizes = [0, 129, 1, 0, 300]
    G, P = len(sizes), sum(sizes)
    a = X.bf16_ints(gen, [P, K], 12)
    w_nk = X.bf16_ints(gen, [G, N, K], 12)
    bias = X.bf16_ints(gen, [G, N], 256)
    rowscale = X.pow2_rowscale(gen, P, -1, 1)
    a2 = X.two_part_ints(gen, [P + 3, r], 2047) / 64               # two-part a2: its split pinned
    b2 = X.bf16_ints(gen, [G, N, r], 4)
    gather2 = torch.randint(0, P + 3, [P], generator=gen, dtype=torch.int32)
    rows = [a[lo:hi] for lo, hi in zip(_offsets(sizes)[:-1], _offsets(sizes)[1:])]
    side = torch.cat([a2[gather2[lo:hi].long()].double() @ b2[g].double().T
                      for g, (lo, hi) in enumerate(zip(_offsets(sizes)[:-1], _offsets(sizes)[1:]))])
    want = _ref(rows, list(w_nk), sizes, bias, rowscale, side)
    X.fits_fp32(float(want.abs().max()) * 2, 1 / 64)
    offsets = torch.tensor(_offsets(sizes), dtype=torch.int32, device=DEV)
    bf = lambda t: t.to(torch.bfloat16).to(DEV)
    args = (bf(a), bf(w_nk.reshape(G * N, K)), offsets, G, N, K, N * K, K, 1, a2.to(DEV), bf(b2), N * r)
    kw = dict(gather2=gather2.to(DEV), bias=bf(bias), rowscale=rowscale.to(DEV))
    if epi == 'plain':
        out = E.grouped_gemm_bf16_ext(*args, **kw)
    elif epi == 'relu':
        out, pre = E.grouped_gemm_bf16_ext(*args, **kw, epilogue=E.EPI_ACT, activation=E.ACT_RELU,
                                           keep_preact=True)
        X.assert_once_rounded(pre, want, 0.0, 'bf16_ext pre-activation')
        want = want.clamp_min(0)
    else:
        base = X.bf16_ints(gen, [P, N], 256) * 8
        out = bf(base)
        E.grouped_gemm_bf16_ext(*args, **kw, out=out, accumulate=True)
        want = want + base.double()
    X.assert_once_rounded(out, want, 0.0, 'grouped_gemm_bf16_ext r={} {}'.format(r, epi))


# ---------------------------------------------------------------------------- lora_down, tall_tn

@pytest.mark.parametrize('exact_flag', [False, True])
@pytest.mark.parametrize('n', [16, 48, 64])
def test_lora_down_is_exact(n, exact_flag):
    E = ext()
    for two_part in ('a', 'w'):
        gen = _gen(n + 2 * exact_flag + (two_part == 'w'))
        K, rows = 160, 1000
        x, t = _operands(gen, two_part, [rows, K], [K, n], K, 0)
        u, img, norms = E.lora_down(x.to(DEV), t.to(DEV), want_image=True, want_norms=True, exact=exact_flag)
        _check(u, x.double() @ t.double(), 'lora_down n={} exact={} {}'.format(n, exact_flag, two_part))
        assert torch.equal(img.buffer, E.split_bf16(x.to(DEV)).buffer), 'the by-product image'
        ub = E.lora_down(x.to(DEV), t.to(DEV), block_major=True, exact=exact_flag)
        _check(ub, (x.double() @ t.double()).view(rows, n // 16, 16).transpose(0, 1), 'lora_down block_major')


def test_lora_down_tables_stacked_grouped_are_exact():
    E = ext()
    gen = _gen(21)
    K, rows = 128, 700
    for two_part in ('a', 'w'):
        x, tabs = _operands(gen, two_part, [rows, K], [3, K, 16], K, 0)
        flat = torch.zeros([3 * (K * 16 + 64)], dtype=torch.float32)
        for j in range(3):
            flat[j * (K * 16 + 64):j * (K * 16 + 64) + K * 16] = tabs[j].reshape(-1)
        flat = flat.to(DEV)
        tables = [flat[j * (K * 16 + 64):j * (K * 16 + 64) + K * 16].view(K, 16) for j in range(3)]
        u, _ = E.lora_down_tables(x.to(DEV), tables)
        _check(u, torch.stack([x.double() @ tabs[j].double() for j in range(3)]), 'lora_down_tables')
        # stacked: G inputs back to back, G tables
        xs_all, _ = _operands(gen, two_part, [3, rows, K], [1], K, 0)
        xs_dev = xs_all.to(DEV)
        out = torch.zeros([rows, 64], device=DEV)
        E.lora_down_stacked([xs_dev[j] for j in range(3)], tables,
                            torch.tensor([0, rows, 2 * rows, 3 * rows], dtype=torch.int32, device=DEV), out)
        want = torch.cat([xs_all[j].double() @ tabs[j].double() for j in range(3)] +
                         [torch.zeros([rows, 16], dtype=torch.float64)], 1)
        _check(out, want, 'lora_down_stacked')
        # grouped: rows sorted by group, one table per group, empty groups
        sizes = [0, 129, 0, 1, 570, 0]
        xg, gt = _operands(gen, two_part, [rows, K], [len(sizes), K, 32], K, 0)
        offsets = torch.tensor(_offsets(sizes), dtype=torch.int32, device=DEV)
        ug = E.lora_down_grouped(xg.to(DEV), gt.to(DEV), offsets)
        want = torch.cat([xg[lo:hi].double() @ gt[g].double()
                          for g, (lo, hi) in enumerate(zip(_offsets(sizes)[:-1], _offsets(sizes)[1:]))])
        _check(ug, want, 'lora_down_grouped')


def test_lora_down_bf16_is_exact():
    E = ext()
    gen = _gen(23)
    K, rows = 192, 900
    x = X.bf16_ints(gen, [rows, K], 32)
    for n in (4, 16, 36, 64):
        t = X.bf16_ints(gen, [K, n], 32)
        u = E.lora_down_bf16(x.bfloat16().to(DEV), t.bfloat16().to(DEV))
        _check(u, x.double() @ t.double(), 'lora_down_bf16 n={}'.format(n))
    sizes = [0, 129, 1, 0, 770, 0]
    tabs = X.bf16_ints(gen, [len(sizes), K, 32], 32)
    offsets = torch.tensor(_offsets(sizes), dtype=torch.int32, device=DEV)
    u = E.lora_down_grouped_bf16(x.bfloat16().to(DEV), tabs.bfloat16().to(DEV), offsets)
    want = torch.cat([x[lo:hi].double() @ tabs[g].double()
                      for g, (lo, hi) in enumerate(zip(_offsets(sizes)[:-1], _offsets(sizes)[1:]))])
    _check(u, want, 'lora_down_grouped_bf16')


def _tall_ref(wide, narrow, gather, sizes):
    nar = narrow[gather.long()] if gather is not None else narrow
    cuts = _offsets(sizes)
    return torch.stack([wide[lo:hi].double().T @ nar[lo:hi].double() for lo, hi in zip(cuts[:-1], cuts[1:])])


@pytest.mark.parametrize('n', [4, 16, 48])
def test_tall_tn_is_exact(n):
    E = ext()
    gen = _gen(n)
    sizes = [0, 1300, 1, 0, 129, 0]
    rows, width = sum(sizes), 96
    offsets = torch.tensor(_offsets(sizes), dtype=torch.int32, device=DEV)
    for two_part in ('a', 'w'):
        wide, narrow = _operands(gen, two_part, [rows, width], [rows + 7, n], rows, 0)
        gather = torch.randint(0, rows + 7, [rows], generator=gen, dtype=torch.int32)
        want = _tall_ref(wide, narrow, gather, sizes)
        got = E.tall_tn(wide.to(DEV), narrow.to(DEV), gather=gather.to(DEV), offsets=offsets)
        _check(got, want, 'tall_tn n={} {}'.format(n, two_part))
        got_t = E.tall_tn(wide.to(DEV), narrow.to(DEV), gather=gather.to(DEV), offsets=offsets, transposed=True)
        _check(got_t, want.transpose(1, 2), 'tall_tn transposed')
        if n % 16 == 0:
            got_s = E.tall_tn(wide.to(DEV), narrow.to(DEV), gather=gather.to(DEV), offsets=offsets, split16=True)
            _check(got_s, want.view(len(sizes), width, n // 16, 16).permute(0, 2, 1, 3), 'tall_tn split16')
        # one group, no gather
        got1 = E.tall_tn(wide.to(DEV), narrow[:rows].to(DEV))
        _check(got1, _tall_ref(wide, narrow[:rows], None, [rows]), 'tall_tn single group')
        wides = [wide.to(DEV), (-wide).to(DEV), wide.flip(0).to(DEV)]
        narrows = [narrow.to(DEV)] * 3
        outs = E.tall_tn_batch(wides, narrows, gather=gather.to(DEV), offsets=offsets)
        for i, o in enumerate(outs):
            _check(o, _tall_ref(wides[i].cpu(), narrow, gather, sizes), 'tall_tn_batch {}'.format(i))


@pytest.mark.parametrize('n', [4, 16, 48])
def test_tall_tn_bf16_stores_rne_of_the_exact_sum(n):
    E = ext()
    gen = _gen(n + 100)
    sizes = [0, 1300, 1, 0, 129, 0]
    rows, width = sum(sizes), 64
    offsets = torch.tensor(_offsets(sizes), dtype=torch.int32, device=DEV)
    wide = X.bf16_ints(gen, [rows, width], 4)
    narrow = X.two_part_ints(gen, [rows + 3, n], 2047) / 256        # the fp32 operand: two-part
    gather = torch.randint(0, rows + 3, [rows], generator=gen, dtype=torch.int32)
    want = _tall_ref(wide, narrow, gather, sizes)
    X.fits_fp32(float(want.abs().max()) * 2, 1 / 256)
    got = E.tall_tn_bf16(wide.bfloat16().to(DEV), narrow.to(DEV), gather=gather.to(DEV), offsets=offsets)
    X.assert_once_rounded(got, want, 0.0, 'tall_tn_bf16 n={}'.format(n))


# ------------------------------------------------------------------------ rows_combine, split_bf16

def test_rows_combine_is_exact():
    E = ext()
    gen = _gen(31)
    T, k, d = 300, 3, 72
    rows = X.two_part_ints(gen, [T * k + 5, d], 40000)
    pos = torch.randperm(T * k + 5, generator=gen)[:T * k].view(T, k).int()
    bias = X.bf16_ints(gen, [d], 256)
    want = rows[pos.long()].double().sum(1) + bias.double()
    _check(E.rows_combine(rows.to(DEV), pos.to(DEV), bias.to(DEV)), want, 'rows_combine')
    side = X.bf16_ints(gen, [T, 5], 16)
    side_w = X.bf16_ints(gen, [5, d], 16)
    _check(E.rows_combine(rows.to(DEV), pos.to(DEV), bias.to(DEV), side=side.to(DEV), side_weight=side_w.to(DEV)),
           want + side.double() @ side_w.double(), 'rows_combine side')
    rb = X.bf16_ints(gen, [T * k + 5, d], 256)
    bb = X.bf16_ints(gen, [d], 256)
    want = rb[pos.long()].double().sum(1) + bb.double()
    X.assert_once_rounded(E.rows_combine(rb.bfloat16().to(DEV), pos.to(DEV), bb.bfloat16().to(DEV)), want, 0.0,
                          'rows_combine bf16')


def test_split_bf16_reproduces_two_part_values():
    E = ext()
    gen = _gen(33)
    rows, cols, ld = 77, 100, 104
    x = torch.full([rows, ld], 3.0)                    # columns past `cols` are not the image's: pad stays 0
    x[:, :cols] = X.two_part_ints(gen, [rows, cols], 65535) * 2.0 ** -7
    img = E.split_bf16(x.to(DEV)[:, :cols])
    blocks = (cols + 31) // 32
    raw = img.buffer.view(torch.bfloat16).view(rows, blocks, 2, 32).cpu()
    hi = raw[:, :, 0].reshape(rows, blocks * 32).double()
    lo = raw[:, :, 1].reshape(rows, blocks * 32).double()
    want = torch.zeros([rows, blocks * 32], dtype=torch.float64)
    want[:, :cols] = x[:, :cols].double()
    _check(hi + lo, want, 'split_bf16 hi + lo (pad columns 0)')
    _check(hi, want.float().bfloat16().double(), 'split_bf16 hi = RNE(x)')
    assert (lo[:, :cols] != 0).float().mean() > 0.9


# ---------------------------------------------------------------------------------- sddmm, spmm

def _csr(gen, B, S, Z):
    idx = torch.stack([torch.stack([torch.randperm(S, generator=gen)[:Z].sort().values for _ in range(S)])
                       for _ in range(B)]).int()
    indptr = (torch.arange(S + 1) * Z).int()
    return indptr, idx.reshape(B, S * Z)


@pytest.mark.parametrize('form', ['matrix_cores', 'gather'])
def test_sddmm_is_exact(form):
    E = ext()
    lib = E.load_library()
    gen = _gen(41)
    B, S, D, Z = (160, 256, 64, 32) if form == 'matrix_cores' else (4, 100, 64, 12)
    assert lib.spt_sddmm_form(B, S, D, S * Z) == (form == 'matrix_cores')
    indptr, idx = _csr(gen, B, S, Z)
    for two_part in ('a', 'w'):
        q, k = _operands(gen, two_part, [B, S, D], [B, S, D], D, 0)
        qd, kd = q.to(DEV), k.to(DEV)
        before = E.paths_taken('sddmm').get(('sddmm', form), 0)
        got = E.sddmm_forward_cuda(False, True, indptr.to(DEV), idx.to(DEV), qd, kd)
        assert E.paths_taken('sddmm').get(('sddmm', form), 0) == before + 1
        cols = idx.view(B, S, Z).long().to(DEV)
        want = torch.einsum('bsd,bszd->bsz', qd.double(), kd.double()[torch.arange(B, device=DEV)[:, None, None], cols])
        _check(got, want.reshape(B, S * Z), 'sddmm {} {}'.format(form, two_part))


@pytest.mark.parametrize('form', ['matrix_cores', 'gather', 'transposed'])
def test_spmm_is_exact(form, monkeypatch):
    E = ext()
    lib = E.load_library()
    monkeypatch.setenv('SPT_SPMM_MFMA', '1' if form == 'matrix_cores' else '0')
    gen = _gen(43)
    B, S, D, Z = (8, 256, 64, 32)
    trans = form == 'transposed'
    if form == 'matrix_cores':
        assert lib.spt_spmm_form(0, B, S, D, S * Z) == 1
    indptr, idx = _csr(gen, B, S, Z)
    for two_part in ('a', 'w'):
        vals, x = _operands(gen, two_part, [B, S * Z], [B, S, D], Z if not trans else 4 * Z, 0)
        key = 'spmm_t' if trans else 'spmm'
        path = 'gather' if trans else form
        before = E.paths_taken(key).get((key, path), 0)
        got = E.spmm_forward_cuda(trans, False, indptr.to(DEV), idx.to(DEV), vals.to(DEV), x.to(DEV))
        assert E.paths_taken(key).get((key, path), 0) == before + 1
        dense = torch.zeros([B, S, S], dtype=torch.float64)
        rows = torch.arange(S).repeat_interleave(Z)
        for b in range(B):
            dense[b].index_put_((rows, idx[b].long()), vals[b].double(), accumulate=True)
        if trans:
            dense = dense.transpose(1, 2)
        want = dense @ x.double()
        _check(got, want, 'spmm {} {}'.format(form, two_part))
