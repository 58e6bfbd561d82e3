"""Frozen base weights stored in fp16: the same bits out, half the memory.

Every comparison is against the library's own fp32-stored path on the same weights, which lie on the
fp16 grid (`w.half().float()`), and the bar is `torch.equal`.  The one exception: where the fp32-stored
path does not reproduce ITSELF bit for bit from run to run (float atomics in no fixed order: the
attention backward inside a model step, which tests/test_gpu_poisoned_buffers.py holds to 1e-5 of
scale, and the captured step, which tests/test_models.py holds to 1e-6), the test runs that path twice,
and only if the two runs differ compares at that named bound.

What "the same kernel paths" means below: the layer-level sites of `ext.paths_taken()` agree, and both
runs make the same number of grouped GEMM launches.  The operand FORM of a GEMM (`('grouped_gemm',
'register' | 'a32' | 'image')`) is not compared: a fp16 weight has no register-operand form, so where
fp32 storage reads the weight through registers (the dX products) fp16 storage reads its image -- the
same MFMAs on the same fragments in the same order, hence the same bits, which is what is asserted.
"""
import gc

import numpy as np
import pytest
import torch
from torch import nn

import test_gpu_guard_bands as bands
import test_gpu_poisoned_buffers as suite
from poison import fresh_caches

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def E():
    from naive_gpt import ext
    ext.load_library()
    return ext


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grid(t):
    return t.half().float()


def _grid_randn(gen, *shape, scale=1.0):
    return _grid(scale * torch.randn(list(shape), generator=gen))


# ---------------------------------------------------------------------------------------------------
# the image

@pytest.mark.parametrize('rows,cols', [(1, 32), (33, 40), (130, 96)])
def test_image_from_halves_is_the_image_of_the_upcast(rows, cols):
    ext = E()
    gen = _gen(rows)
    ld = (cols + 7) // 8 * 8 + 8                       # a row stride larger than cols (16-byte rows of halves)
    base = (4.0 * torch.randn([rows, ld], generator=gen)).half()
    vals = base[:, :cols].reshape(-1)
    special = torch.tensor([65504.0, -65504.0, 0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -15 - 2.0 ** -24,
                            2.0 ** -14, 1.0 + 2.0 ** -10, -(2.0 - 2.0 ** -10)], dtype=torch.float16)
    # (fp16 subnormals: 2^-24 the smallest, 2^-15 - 2^-24 inside the range; +-max; both zeros)
    at = torch.randperm(vals.numel(), generator=gen)[:special.numel()]
    flat = base.view(-1)
    for i, v in zip(at.tolist(), special):
        flat[(i // cols) * ld + i % cols] = v
    base[:, cols:] = 3.0                               # behind `cols`: not the image's, its pad stays 0
    assert (base[:, :cols].float().abs() < 2.0 ** -14).any() and torch.signbit(base[:, :cols]).any()
    h = base.to(DEV)[:, :cols]
    f = base.float().to(DEV)[:, :cols]
    assert h.stride(0) == ld and f.stride(0) == ld
    got, want = ext.split_bf16(h), ext.split_bf16(f)
    assert (got.rows, got.cols) == (want.rows, want.cols) == (rows, cols)
    assert got.buffer.numel() == rows * ((cols + 31) // 32) * 128
    assert torch.equal(got.buffer, want.buffer)
    # hi + lo == x exactly, pad columns zero (read back through the layout of include/spt_hip.h)
    img = want.buffer.view(torch.bfloat16).view(rows, -1, 2, 32).float()
    back = (img[:, :, 0] + img[:, :, 1]).reshape(rows, -1)
    assert torch.equal(back[:, :cols], f) and (back[:, cols:] == 0).all()
    assert torch.equal(ext.weight_image(h.contiguous()).buffer, want.buffer)      # the contiguous twin
    fresh_caches()


# ---------------------------------------------------------------------------------------------------
# the GEMM: fp16 `weight` against fp32 `weight`

P, K, N, G = 256, 64, 160, 2
SIZES = [0, 256]                                        # one empty group: the second group's offset is live
R = 16


def _queue_count(ext):
    return int(ext.LAST_RELU_QUEUE[:256 * 64].view(torch.int32).view(256, 16)[:, 0].sum())


def _operands(kink=False):
    """a [P, K] fp32, w [G, N, K] on the fp16 grid (k contiguous), and the rest of a fused call.
    `kink`: rows 0 .. 7 of `a` all zero (pre-activation exactly 0 with no bias) and rows 8 .. 71 turned,
    in fp64, until their product with weight row n = p lies 1e-3 .. 3e-5 from zero -- inside the kernel's window
    (2.29e-5 |a| |w| ~ 1.5e-3 here) and above the error of a plain fp32 dot product (3e-7 |a| |w| ~ 2e-5):
    cells whose sign only the fp32 recomputation decides, from operands it really has to read."""
    gen = _gen(5)
    a = torch.randn([P, K], generator=gen)
    w = _grid_randn(gen, G, N, K)
    if kink:
        a64, w64 = a.double(), w.double()[1]            # every row is in group 1
        for p in range(8, 72):
            nudge = (1 if p % 2 else -1) * 10.0 ** (-3.0 - 1.5 * (p - 8) / 64)
            a64[p] -= (w64[p] @ a64[p] - nudge) / (w64[p] @ w64[p]) * w64[p]
        a = a64.float()
        a[:8] = 0.0
    return dict(a=a.to(DEV), w=w.to(DEV), a2=torch.randn([P, R], generator=gen).to(DEV),
                b2=torch.randn([G, N, R], generator=gen).to(DEV), bias=torch.randn([G, N], generator=gen).to(DEV),
                scale=(torch.rand([P], generator=gen) + 0.5).to(DEV), s=torch.randn([P, N], generator=gen).to(DEV),
                prior=torch.randn([P, N], generator=gen).to(DEV),
                off=torch.tensor(np.concatenate([[0], np.cumsum(SIZES)]), dtype=torch.int32).to(DEV))


def _both(call, o, bn=False):
    """call(weight, w_image) with the fp32 weight and with its halves -> (fp32 outputs, fp16 outputs, the
    fp32 run's ReLU-queue count or None); the operand form must be an image form both times."""
    ext = E()
    w32 = o['w'].transpose(1, 2).contiguous() if bn else o['w']       # [G, K, N]: n contiguous
    w16 = w32.half()
    assert torch.equal(w16.float(), w32)
    outs = []
    for w in (w32, w16):
        fresh_caches()
        ext.LAST_RELU_QUEUE = None
        out = call(w, ext.split_bf16(w.view(-1, w.size(-1))))
        torch.cuda.synchronize()
        assert ext.LAST_GEMM_PATH == 'a32', ext.LAST_GEMM_PATH
        outs.append([t.clone() for t in suite._flatten(out)])
        if w is w32:
            count = _queue_count(ext) if ext.LAST_RELU_QUEUE is not None else None
    return outs[0], outs[1], count


def _same(got, want, what):
    assert len(got) == len(want) and len(want) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and torch.isfinite(w).all(), (what, i)
        assert torch.equal(g, w), '{}: output {} from the fp16 weight differs from the fp32 weight\'s in {} of {} ' \
            'elements (max {:.3e})'.format(what, i, int((g != w).sum()), w.numel(), float((g - w).abs().max()))


@pytest.mark.parametrize('bn', [False, True], ids=['w_ldk_1', 'w_ldn_1'])
def test_gemm_plain_both_orientations(bn):
    ext, o = E(), _operands()
    strides = dict(w_group_stride=N * K, w_ldn=1, w_ldk=N) if bn else dict(w_group_stride=N * K, w_ldn=K, w_ldk=1)

    def call(w, img):
        return ext.grouped_gemm_fused(o['a'], w, o['off'], G, n=N, k=K, n_rows=P, bias=o['bias'],
                                      rowscale=o['scale'], w_image=img, **strides)
    want, got, _ = _both(call, o, bn)
    _same(got, want, 'EPI_PLAIN')
    ref = o['scale'][:, None] * (o['a'] @ o['w'][1].T + o['bias'][1])
    assert (want[0] - ref).abs().max() <= 1e-4 * ref.abs().max()          # (the right product at all)


def test_gemm_k_extension_and_accumulate():
    ext, o = E(), _operands()

    def call(w, img):
        out = o['prior'].clone()
        return ext.grouped_gemm_fused(o['a'], w, o['off'], G, n=N, k=K, w_group_stride=N * K, w_ldn=K, w_ldk=1,
                                      n_rows=P, rowscale=o['scale'], a2=o['a2'], b2=o['b2'], b2_group_stride=N * R,
                                      w_image=img, out=out, accumulate=True)
    want, got, _ = _both(call, o)
    _same(got, want, 'K extension + accumulate')
    assert not torch.equal(want[0], o['prior'])


def test_gemm_dact():
    ext, o = E(), _operands()

    def call(w, img):
        return ext.grouped_gemm_fused(o['a'], w, o['off'], G, n=N, k=K, w_group_stride=N * K, w_ldn=K, w_ldk=1,
                                      n_rows=P, rowscale=o['scale'], a2=o['a2'], b2=o['b2'], b2_group_stride=N * R,
                                      epilogue=ext.EPI_DACT, activation=ext.ACT_SILU, s_in=o['s'], w_image=img,
                                      raw_dots=True)
    want, got, _ = _both(call, o)
    assert len(want) == 3
    _same(got, want, 'EPI_DACT')


def test_gemm_act_silu():
    ext, o = E(), _operands()

    def call(w, img):
        return ext.grouped_gemm_fused(o['a'], w, o['off'], G, n=N, k=K, w_group_stride=N * K, w_ldn=K, w_ldk=1,
                                      n_rows=P, bias=o['bias'], rowscale=o['scale'], a2=o['a2'], b2=o['b2'],
                                      b2_group_stride=N * R, epilogue=ext.EPI_ACT, activation=ext.ACT_SILU,
                                      keep_preact=True, w_image=img)
    want, got, _ = _both(call, o)
    assert len(want) == 2
    _same(got, want, 'EPI_ACT SiLU')


@pytest.mark.parametrize('entries', [None, 256], ids=['queue', 'queue_full_epilogue_recomputes'])
def test_gemm_act_relu_at_the_kink(entries):
    """Cells at the kink: all-zero rows of `a` without a bias (pre-activation exactly 0) and cells turned
    to within 3e-5 .. 1e-3 of zero (`_operands`).  `entries` = 256: one slot per queue segment, so all but a handful of
    the cells are recomputed in the epilogue itself (`gg_exact_preact` inlined there); None: by
    relu_fix_kernel.  Both read the weight's halves."""
    ext, o = E(), _operands(kink=True)

    def call(w, img):
        return ext.grouped_gemm_fused(o['a'], w, o['off'], G, n=N, k=K, w_group_stride=N * K, w_ldn=K, w_ldk=1,
                                      n_rows=P, epilogue=ext.EPI_ACT, activation=ext.ACT_RELU, keep_preact=True,
                                      w_image=img, relu_queue_entries=entries)
    want, got, count = _both(call, o)
    assert count is not None and count >= 8 * N + 64, 'the fp32 run queued {} cells: the exact path did not run'.format(count)
    if entries is not None:
        assert count > 8 * entries // 256 * 8, 'the queue did not overflow ({} cells): nothing was recomputed in ' \
            'the epilogue'.format(count)
    _same(got, want, 'EPI_ACT ReLU')
    h, pre = want
    assert (pre[:8] == 0).all() and torch.equal(h, pre.clamp_min(0.0))
    # the turned cells carry the fp32 dot product's sign, which is fp64's
    p = torch.arange(8, 72)
    a64, w64 = o['a'].double().cpu()[p], o['w'].double().cpu()[1][p]
    exact = (a64 * w64).sum(-1)
    decided = exact.abs() > 3e-7 * a64.norm(dim=1) * w64.norm(dim=1)      # beyond the fp32 recomputation's error
    assert (exact.abs() < 2e-3).all() and decided.sum() >= 32            # (rounding `a` to fp32 moves a cell by ~4e-6)
    assert ((pre.cpu()[p, p] > 0) == (exact > 0))[decided].all(), 'a ReLU sign differs from fp64'
    assert (exact.abs() <= 2.2888e-5 * a64.norm(dim=1) * w64.norm(dim=1)).all()      # inside the kernel's window


def test_fp16_weight_off_the_image_path_is_refused():
    ext, o = E(), _operands()
    w16 = o['w'].half()
    with pytest.raises(RuntimeError, match='image path'):
        ext.grouped_gemm_fused(o['a'], w16, o['off'], G, n=N, k=K, w_group_stride=N * K, w_ldn=K, w_ldk=1, n_rows=P)
    k = 48                                               # not a whole number of k-steps: register path only
    a, w = o['a'][:, :k].contiguous(), w16[:, :, :k].contiguous()
    with pytest.raises(RuntimeError, match='image path'):
        ext.grouped_gemm_fused(a, w, o['off'], G, n=N, k=k, w_group_stride=N * k, w_ldn=k, w_ldk=1, n_rows=P,
                               w_image=ext.split_bf16(w.view(-1, k)))
    # ... which the fp32 weight takes (through registers)
    ext.grouped_gemm_fused(a, w.float(), o['off'], G, n=N, k=k, w_group_stride=N * k, w_ldn=k, w_ldk=1, n_rows=P,
                           w_image=ext.split_bf16(w.float().view(-1, k)))
    assert ext.LAST_GEMM_PATH == 'register'
    torch.cuda.synchronize()


# the segmented contraction (the joint dX of q / k / v): K walks three matrices lying apart, the second term
# is 48 wide in three 16-column tables lying apart.  fp32 storage runs it through registers; halves run it
# from the weight's image and the activation's fp32 rows, to the same bits.
SEG_ROWS, SEG_N = 200, 160                              # two row tiles, the second ragged; N no multiple of 128


def _segmented(seg_k, bn, second_term, dev=None):
    gen = _gen(11 + seg_k)
    dev = dev or (lambda t: t.to(DEV))
    k = 3 * seg_k
    buf = dev(torch.randn([3, SEG_ROWS + 5, seg_k], generator=gen))          # (5 rows between the matrices)
    w = _grid_randn(gen, k, SEG_N) if bn else _grid_randn(gen, SEG_N, k)
    kw = dict(w_group_stride=0, w_ldn=1, w_ldk=SEG_N) if bn else dict(w_group_stride=0, w_ldn=k, w_ldk=1)
    kw.update(a_segments=(seg_k, (SEG_ROWS + 5) * seg_k))
    tables = du = None
    if second_term:
        du = dev(torch.randn([SEG_ROWS, 48], generator=gen))
        tables = dev(torch.randn([3, SEG_N + 3, 16], generator=gen))
        kw.update(a2=du, b2=tables[0, :SEG_N], b2_segment_stride=(SEG_N + 3) * 16)
    one = dev(torch.tensor([0, SEG_ROWS], dtype=torch.int32))
    want = sum(buf[g, :SEG_ROWS].double().cpu() @ (w[g * seg_k:(g + 1) * seg_k] if bn else
                                                   w[:, g * seg_k:(g + 1) * seg_k].T).double() for g in range(3))
    if second_term:
        want = want + sum(du[:, 16 * g:16 * g + 16].double().cpu() @ tables[g, :SEG_N].double().cpu().T
                          for g in range(3))

    def call(weight, **more):
        return E().grouped_gemm_fused(buf[0, :SEG_ROWS], weight, one, 1, n=SEG_N, k=k, n_rows=SEG_ROWS, **kw, **more)
    return call, dev(w), want


@pytest.mark.parametrize('second_term', [False, True], ids=['plain', 'second_term_48'])
@pytest.mark.parametrize('bn', [False, True], ids=['w_ldk_1', 'w_ldn_1'])
@pytest.mark.parametrize('seg_k', [32, 64])
def test_gemm_segmented_contraction(seg_k, bn, second_term):
    ext = E()
    call, w32, want64 = _segmented(seg_k, bn, second_term)
    w16 = w32.half()
    assert torch.equal(w16.float(), w32)
    want = call(w32)
    assert ext.LAST_GEMM_PATH == 'register'
    got = call(w16, w_image=ext.split_bf16(w16))
    torch.cuda.synchronize()
    assert ext.LAST_GEMM_PATH == 'a32'
    _same([got], [want], 'segmented contraction')
    assert (want.double().cpu() - want64).abs().max() <= 1e-4 * want64.abs().max()      # (the right product at all)
    with pytest.raises(RuntimeError, match='image path'):                    # halves: never without the image
        call(w16)
    fresh_caches()


# ---------------------------------------------------------------------------------------------------
# poisoned buffers and guard bands: the new operand forms through tests/poison.py and tests/guard.py

def _split_f16_case():
    ext = E()
    gen = _gen(7)
    base = torch.randn([33, 48], generator=gen).half()
    x = suite._dev(base)[:, :40]                         # ragged last block, rows 96 bytes apart

    def call():
        return ext.split_bf16(x)

    def check(outs):
        img = outs[0].view(torch.bfloat16).view(33, 2, 2, 32).float()
        back = (img[:, :, 0] + img[:, :, 1]).reshape(33, 64)
        assert torch.equal(back[:, :40].cpu(), base[:, :40].float()) and (back[:, 40:] == 0).all()
    return call, check


def _gemm_w16_case():
    ext = E()
    o = _operands(kink=True)
    a, w16, off = suite._dev(o['a'].cpu()), suite._dev(o['w'].cpu().half()), suite._dev(o['off'].cpu())

    def call():
        h, pre = ext.grouped_gemm_fused(a, w16, off, G, n=N, k=K, w_group_stride=N * K, w_ldn=K, w_ldk=1,
                                        n_rows=P, epilogue=ext.EPI_ACT, activation=ext.ACT_RELU,
                                        keep_preact=True, w_image=ext.split_bf16(w16.view(-1, K)))
        assert ext.LAST_GEMM_PATH == 'a32'
        counts = ext.LAST_RELU_QUEUE[:256 * 64].view(torch.int32).view(256, 16)[:, 0].clone()
        return h, pre, counts

    def check(outs):
        h, pre, counts = outs
        want = suite._ref_grouped(a, w16.float().view(G * N, K), SIZES, N, K)
        suite._close(pre, want, 'preact', rtol=1e-5)
        assert int(counts.sum()) >= 8 * N + 64 and torch.equal(h, pre.clamp_min(0.0))
    return call, check


def _gemm_w16_segmented_case():
    ext = E()
    call, w32, want64 = _segmented(32, True, True, dev=suite._dev)
    w16 = suite._dev(w32.cpu().half())

    def run():
        out = call(w16, w_image=ext.split_bf16(w16))
        assert ext.LAST_GEMM_PATH == 'a32'
        return out

    def check(outs):
        suite._close(outs[0], want64.float(), 'segmented', rtol=1e-4)
    return run, check


NEW_FORMS = [('split_bf16', suite.Case('from_fp16_cols_40', _split_f16_case, suite.DET)),
             ('grouped_gemm_fused', suite.Case('fp16_weight_relu_near_kink', _gemm_w16_case, suite.DET)),
             ('grouped_gemm_fused', suite.Case('fp16_weight_segmented', _gemm_w16_segmented_case, suite.DET))]


@pytest.mark.parametrize('entry,case', NEW_FORMS, ids=[c.name for _, c in NEW_FORMS])
def test_new_operand_forms_ignore_what_their_buffers_held(entry, case):
    suite.test_entry_ignores_what_its_buffers_held(entry, case)


@pytest.mark.parametrize('entry,case', NEW_FORMS, ids=[c.name for _, c in NEW_FORMS])
def test_new_operand_forms_stay_inside_their_buffers(entry, case):
    bands.test_entry_stays_inside_its_buffers(entry, case)


# ---------------------------------------------------------------------------------------------------
# layers

F16_NOTES = ('f16_upcast',)


def _kernel_paths(paths):
    """(layer-level sites and their paths, grouped GEMM launches, the fp16 fallback notes)"""
    sites = {k: v for k, v in paths.items() if k[0] != 'grouped_gemm' and k[1] not in F16_NOTES}
    gemms = sum(v for k, v in paths.items() if k[0] == 'grouped_gemm')
    notes = {k: v for k, v in paths.items() if k[1] in F16_NOTES}
    return sites, gemms, notes


def _layer_runs(make, inputs, grads, forward=None):
    """make() -> a module with frozen weights on the fp16 grid.  Runs it in fp32 storage twice and in
    fp16 storage once on the same inputs -> three ([outputs, input grads, parameter grads], paths)."""
    from naive_gpt import utils
    ext = E()
    runs = []
    for stored in (False, False, True):
        torch.manual_seed(0)
        m = make().to(DEV)
        if stored:
            report = utils.store_frozen_fp16(m)
            assert report['converted'] and not report['kept'], report
        xs = [x.clone().requires_grad_(True) for x in inputs]
        fresh_caches()
        ext.reset_paths()
        ys = forward(m, *xs) if forward else m(*xs)
        ys = list(ys) if isinstance(ys, (tuple, list)) else [ys]
        torch.autograd.backward(ys, [g[:y.numel()].view(y.shape) for y, g in zip(ys, grads)])
        torch.cuda.synchronize()
        named = [(n, p.grad) for n, p in m.named_parameters() if p.grad is not None]
        assert all(p.dtype == (torch.float16 if stored else torch.float32)
                   for n, p in m.named_parameters() if n.endswith('weight') and not p.requires_grad and p.dim() == 2
                   and 'lora' not in n and 'router' not in n)
        runs.append(([y.detach().clone() for y in ys] + [x.grad.clone() for x in xs] + [g.clone() for _, g in named],
                     [n for n, _ in named], dict(ext.paths_taken())))
    return runs


def _assert_layer(runs, what, n_grads, allowed_notes=()):
    (base, names, paths), (again, _, _), (got, names16, paths16) = runs
    assert names == names16 and len(names) >= n_grads, names
    for a, b in zip(base, again):
        assert torch.equal(a, b), what + ': the fp32-stored layer does not reproduce itself'
    for i, (g, w) in enumerate(zip(got, base)):
        assert torch.isfinite(w).all() and w.abs().max() > 0, (what, i)
        assert torch.equal(g, w), '{}: tensor {} of {} differs between fp16 and fp32 storage: {} elements, ' \
            'max {:.3e}'.format(what, i, ['outputs / input grads'] + names, int((g != w).sum()),
                                float((g - w).abs().max()))
    sites, gemms, notes = _kernel_paths(paths)
    sites16, gemms16, notes16 = _kernel_paths(paths16)
    assert sites16 == sites, (what, sorted(set(sites16.items()) ^ set(sites.items())))
    assert gemms16 == gemms
    assert not notes and set(notes16) == set(allowed_notes), (what, notes16)
    return paths, paths16


def _reasons(site):
    """Has `ext` forget the fallback reasons logged so far (it keeps a few per site, and other tests of
    the process may have filled that) -> a function returning those logged since for `site`'s fp16 upcast."""
    ext = E()
    ext.reset_paths(reasons=True)
    return lambda: ext.fallback_reasons(site, 'f16_upcast')


def _random_tables(m, gen):
    for name, p in m.named_parameters():
        if name.endswith('lora.right.weight'):               # a fresh adapter is the identity
            p.data.copy_(0.1 * torch.randn(p.shape, generator=gen))
    for name, p in m.named_parameters():
        if not p.requires_grad:
            p.data.copy_(_grid(p.data))
    return m


def _lora_linear():
    from naive_gpt import layers
    return _random_tables(layers.LoRALinear(d_lora=16, in_features=64, out_features=96), _gen(1))


def test_lora_linear_2048_rows():
    gen = _gen(2)
    x = torch.randn([2048, 64], generator=gen).to(DEV)
    g = torch.randn([2048 * 96], generator=gen).to(DEV)
    runs = _layer_runs(_lora_linear, [x], [g])
    paths, paths16 = _assert_layer(runs, 'LoRALinear 64 -> 96', 2)
    assert paths[('lora_linear', 'mfma')] == 1 and paths[('lora_linear_backward', 'mfma')] == 1
    assert sum(v for k, v in paths16.items() if k[0] == 'grouped_gemm') == 2
    assert ('grouped_gemm', 'register') not in paths16 and ('lora_linear', 'library') not in paths16


def test_lora_linear_512_rows_notes_its_fallback():
    gen = _gen(3)
    x = torch.randn([512, 64], generator=gen).to(DEV)
    g = torch.randn([512 * 96], generator=gen).to(DEV)
    reasons = _reasons('lora_linear')
    runs = _layer_runs(_lora_linear, [x], [g])
    _assert_layer(runs, 'LoRALinear at 512 rows', 2,
                  allowed_notes=[('lora_linear', 'f16_upcast'), ('lora_linear_backward', 'f16_upcast')])
    paths16 = runs[2][2]
    assert paths16[('lora_linear', 'library')] == 1 and paths16[('lora_linear', 'f16_upcast')] == 1
    why = reasons()
    assert why and all('fp16-stored' in w and '2048 rows' in w for w in why), why


class _QKV(nn.Module):
    def __init__(self):
        from naive_gpt import layers
        super().__init__()
        self.linear_q, self.linear_k, self.linear_v = [
            layers.LoRALinear(d_lora=16, in_features=64, out_features=96) for _ in range(3)]

    def forward(self, x):
        from naive_gpt.layers.tuning import lora
        linears = [self.linear_q, self.linear_k, self.linear_v]
        assert lora.qkv_usable(x, linears)
        return lora.qkv(x, linears)


def test_joint_qkv_of_a_self_attention():
    """The joint dX = [dQ | dK | dV] [Wq; Wk; Wv] walks K in segments with a 48-wide second term: fp32
    storage reads the three homed weights through registers, fp16 storage their one image
    (test_gemm_segmented_contraction) -- no upcast, no fallback note."""
    gen = _gen(4)
    x = torch.randn([2048, 64], generator=gen).to(DEV)
    g = torch.randn([3, 2048 * 96], generator=gen).to(DEV)          # dQ, dK, dV equally spaced: the joint dX
    runs = _layer_runs(lambda: _random_tables(_QKV(), _gen(5)), [x], [g[0], g[1], g[2]])
    paths, paths16 = _assert_layer(runs, 'joint q / k / v', 6)
    assert paths[('qkv_dx', 'joint')] == 1 and paths16[('qkv_dx', 'joint')] == 1
    assert ('qkv_dx', 'three_launches') not in paths16 and ('grouped_gemm', 'register') not in paths16


def test_joint_qkv_keeps_one_image_of_the_three_weights(monkeypatch):
    """SPT_WEIGHT_IMAGES=keep: the one image of the three homed fp16 weights is made once and serves the
    forward and the joint dX of every later step (the layer hands `ext.weight_image` the same view each time)."""
    ext = E()
    gen = _gen(4)
    x = torch.randn([2048, 64], generator=gen).to(DEV)
    g = torch.randn([3, 2048 * 96], generator=gen).to(DEV)
    from naive_gpt import utils
    torch.manual_seed(0)
    m = _random_tables(_QKV(), _gen(5)).to(DEV)
    utils.store_frozen_fp16(m)
    fresh_caches()
    made, split = [], ext.split_bf16
    monkeypatch.setattr(ext, 'split_bf16', lambda t: made.append((t.dtype, tuple(t.shape))) or split(t))
    results = []
    for keep in (False, True, True):
        monkeypatch.setattr(ext, 'KEEP_WEIGHT_IMAGES', keep)
        xs = x.clone().requires_grad_(True)
        del made[:]
        ys = m(xs)
        torch.autograd.backward(list(ys), [g[i].view(ys[i].shape) for i in range(3)])
        torch.cuda.synchronize()
        results.append((xs.grad.clone(), list(made)))
        m.zero_grad(set_to_none=True)
    joint = (torch.float16, (3 * 96, 64))
    assert results[0][1].count(joint) == 2 and results[1][1].count(joint) == 1 and results[2][1].count(joint) == 0
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][0], results[2][0])
    fresh_caches()


def _routed(kind, block=64, d_lora=16):
    from naive_gpt import layers
    if kind == 'opt':
        m = layers.LoRARoutedFFN(d_lora=d_lora, block_size=block, d_model=64, d_feedforward=4 * block,
                                 activation=nn.ReLU())
    else:
        m = layers.LoRARoutedLLaMaFFN(d_lora=d_lora, block_size=block, d_model=64, d_feedforward=4 * block,
                                      activation=nn.SiLU())
    return _random_tables(m, _gen(6))


@pytest.mark.parametrize('block', [32, 64])
@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_lora_routed_ffn(kind, block):
    """d_model 64, four blocks, 200 tokens (ragged buckets, more than one row tile).  Block size 32 is the
    smallest at which the layer is fused and the edge of the image path's `% 32`: a block's weight rows are
    ONE 32-element image block and group offsets fall on odd blocks; 64 is the smallest the repository's
    own fused-layer tests use.  Outputs, the input gradient and every table / router gradient."""
    gen = _gen(8)
    x = torch.randn([200, 64], generator=gen).to(DEV)
    g = torch.randn([200 * 64], generator=gen).to(DEV)
    runs = _layer_runs(lambda: _routed(kind, block), [x], [g])
    paths, paths16 = _assert_layer(runs, 'LoRA routed FFN ' + kind, 6 if kind == 'opt' else 8)
    assert suite._sites(paths, 'routed_ffn') == suite._sites(paths16, 'routed_ffn') == {'fused'}
    assert ('grouped_gemm', 'register') not in paths16
    names = runs[0][1]
    assert any('router' in n for n in names) and sum('lora' in n for n in names) >= (4 if kind == 'opt' else 6)


@pytest.mark.parametrize('d_lora', [6, 48])
@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_lora_routed_ffn_off_the_fused_path(kind, d_lora):
    """A rank the fused epilogues do not take (not a multiple of 4; above 32): the layer runs its
    `grouped_linear` composition, in fp32 storage as before, and in fp16 storage on transient fp32 copies
    of its block weights -- noted, and to the same bits."""
    gen = _gen(9)
    x = torch.randn([200, 64], generator=gen).to(DEV)
    g = torch.randn([200 * 64], generator=gen).to(DEV)
    reasons = _reasons('routed_ffn')
    runs = _layer_runs(lambda: _routed(kind, 64, d_lora), [x], [g])
    paths, paths16 = _assert_layer(runs, 'LoRA routed FFN {} rank {}'.format(kind, d_lora),
                                   6 if kind == 'opt' else 8, allowed_notes=[('routed_ffn', 'f16_upcast')])
    assert suite._sites(paths, 'routed_ffn') == {'grouped_linear'}
    assert suite._sites(paths16, 'routed_ffn') == {'grouped_linear', 'f16_upcast'}
    assert paths16[('routed_ffn', 'f16_upcast')] == (2 if kind == 'opt' else 3)
    why = reasons()
    assert why and all('fp16-stored' in w and 'fused grouped path' in w for w in why), why


def test_bf16_modules_are_refused_with_a_reason():
    from naive_gpt import utils
    m = _routed('opt').to(DEV)
    utils.store_frozen_fp16(m)
    with pytest.raises(RuntimeError, match='fp32 modules only'):
        m(torch.zeros([64, 64], dtype=torch.bfloat16, device=DEV))
    lin = _lora_linear().to(DEV).bfloat16()
    report = utils.store_frozen_fp16(lin)
    assert not report['converted'] and 'bfloat16' in report['kept']['weight']


# ---------------------------------------------------------------------------------------------------
# the model

CONFIG = dict(d_model=256, n_heads=4, n_layers=2, max_length=128, vocab_size=512, d_feedforward=1024, p_dropout=0.0)
BATCH = 16                                              # 2048 tokens: the matrix-core linears, the fused head loss


def _tuner(kind, stored):
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    torch.manual_seed(0)
    model = utils.upgrade_sparse(checkpoint.build_model(kind, dict(CONFIG)), d_lora=16)
    gen = _gen(40)
    for name, p in model.named_parameters():
        if name.endswith('lora.right.weight'):
            p.data.copy_(0.05 * torch.randn(p.shape, generator=gen))
        else:
            p.data.copy_(_grid(p.data))                 # a checkpoint published in fp16, upcast
    return utils.SparseTuner(model.to(DEV), frozen_fp16=stored)


def _batches(n):
    gen = _gen(41)
    return [torch.randint(3, CONFIG['vocab_size'], [BATCH, CONFIG['max_length'] + 2], generator=gen).to(DEV)
            for _ in range(n)]


def _session(kind, stored, batches):
    """Two training steps of a fresh tuner -> (losses, trained parameters, bytes the tuner holds on the
    device once the steps' temporaries are gone, the conversion report, paths)."""
    ext = E()
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    tuner = _tuner(kind, stored)
    fresh_caches()
    ext.reset_paths()
    losses = [tuner.training_step(b).clone() for b in batches]
    torch.cuda.synchronize()
    paths = dict(ext.paths_taken())
    params = {n: p.detach().cpu().clone() for n, p in tuner.model.named_parameters() if p.requires_grad}
    losses = [l.cpu() for l in losses]
    tuner.model.zero_grad(set_to_none=True)
    fresh_caches()
    gc.collect()
    held = torch.cuda.memory_allocated() - base
    report = tuner.frozen_fp16_report
    tuner.release()
    del tuner
    gc.collect()
    return losses, params, held, report, paths


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_tuner_with_frozen_fp16_trains_to_the_same_bits_in_less_memory(kind):
    batches = _batches(2)
    # (fp16 storage first: the package's small index caches are then allocated in ITS session and count
    # against the saving, not for it)
    l16, p16, held16, report, paths16 = _session(kind, True, batches)
    l32, p32, held32, none, paths32 = _session(kind, False, batches)
    l32b, p32b, _, _, _ = _session(kind, False, batches)
    assert none is None and len(report['converted']) == 2 * (4 + (2 if kind == 'opt' else 3)) and not report['kept']
    assert suite._sites(paths32, 'routed_ffn') == suite._sites(paths16, 'routed_ffn') == {'fused'}, sorted(paths16)
    assert paths16.get(('lora_linear', 'mfma'), 0) > 0 and ('lora_linear', 'library') not in paths16
    sites32, gemms32, notes32 = _kernel_paths(paths32)
    sites16, gemms16, notes16 = _kernel_paths(paths16)
    assert sites16 == sites32 and gemms16 == gemms32 and not notes32 and not notes16, notes16
    reproducible = all(torch.equal(a, b) for a, b in zip(l32, l32b)) and all(torch.equal(p32[n], p32b[n]) for n in p32)
    print('[frozen_f16] {}: fp32-stored step reproducible bit for bit: {}; held {} -> {} bytes, freed {}'.format(
        kind, reproducible, held32, held16, report['bytes_freed']))
    assert p16.keys() == p32.keys() and len(p32) > 20
    if reproducible:
        for a, b in zip(l16, l32):
            assert torch.equal(a, b), (l16, l32)
        for n in p32:
            assert torch.equal(p16[n], p32[n]), n
    else:
        # the attention backward's float atomics: the bound of tests/test_models.py
        # test_captured_step_replays_the_eager_step for two runs of one step sequence -- losses to 1e-6
        # relative, trained parameters to rtol 1e-6 / atol 1e-7
        for a, b in zip(l16, l32):
            assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b)), (l16, l32)
        for n in p32:
            assert torch.allclose(p16[n], p32[n], rtol=1e-6, atol=1e-7), n
    # half the fp32 bytes of the converted tensors, less allocator rounding (< 1 % for tensors of 64 KiB
    # and more; these are 256 KiB and 1 MiB): the 0.9 is a condition, not a measurement
    assert held32 - held16 >= 0.9 * report['bytes_freed'], (held32, held16, report['bytes_freed'])


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_captured_step_with_frozen_fp16_replays_the_eager_step(kind):
    """One captured and replayed step against the eager step of an identical tuner, both in fp16
    storage, at the bound of tests/test_models.py test_captured_step_replays_the_eager_step (losses 1e-6
    relative, parameters rtol 1e-6 / atol 1e-7: the attention backward's atomics)."""
    warm, batch = _batches(2)
    eager, graphed = _tuner(kind, True), _tuner(kind, True)
    try:
        eager.use_capturable_optimizer()
        graphed.capture(batch.shape, pq_loss=True, warmup=3, example=warm)
        for _ in range(3):
            eager.training_step(warm, pq_loss=True)
        le = float(eager.training_step(batch, pq_loss=True))
        lg = float(graphed.training_step(batch, pq_loss=True))
        torch.cuda.synchronize()
        assert graphed._graph is not None and abs(le - lg) <= 1e-6 * abs(le), (le, lg)
        for (n, pe), pg in zip(eager.model.named_parameters(), graphed.model.parameters()):
            if pe.requires_grad:
                assert torch.allclose(pe, pg, rtol=1e-6, atol=1e-7), n
            elif n in eager.frozen_fp16_report['converted']:
                assert pe.dtype == torch.float16 and torch.equal(pe, pg), n
        assert len(eager.frozen_fp16_report['converted']) == 2 * (4 + (2 if kind == 'opt' else 3))
    finally:
        eager.release()
        graphed.release()
        fresh_caches()
