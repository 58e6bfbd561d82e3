"""Every HIP entry of naive_gpt.ext on poisoned buffers: no result may depend on what the memory
the library allocates held before the call (tests/poison.py).

Each case of CASES runs twice under the `zero` pattern and once under `nan` and `big`:

* DET cases give the same bits twice under `zero`; their poisoned runs must give the same bits
  again, in every output.
* ATOMIC cases sum with float atomics in no fixed order (grad_table of cdist.hip:178, grad_k /
  grad_v of mfma_attention.hip: attention_mfma_backward_keys_kernel): their poisoned runs must be
  NaN-free and pass the same reference check as the `zero` run.

The class is part of the registry: a DET case that starts to vary fails.  The `zero` run is
compared with an fp64 or oracle reference, and where the mathematics gives exact zeros (empty
groups, keys no query attends, rows no id names) they are asserted exactly.
"""
import collections
import contextlib
import os

import numpy as np
import pytest
import torch

from poison import PATTERNS, fresh_caches, poisoned, same_bits

pytestmark = pytest.mark.gpu

DET, ATOMIC = 'deterministic', 'order-nondeterministic'
Case = collections.namedtuple('Case', 'name build kind')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t):
    """Every operand of every case reaches the device through this one function, so that
    test_gpu_guard_bands can swap it for guard.home: an input then lies between guard bands, as the
    wrappers' own allocations do (test_poison_coverage checks that no case bypasses it)."""
    return t.cuda()


def _randn(gen, *shape, dtype=torch.float32):
    return _dev(torch.randn(list(shape), generator=gen).to(dtype))


def _offsets(sizes):
    return _dev(torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32))


def _close(got, want, name, rtol=1e-4, atol=0.0):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(want.abs().max().item(), 1e-30) if want.numel() else 1.0
    err = (got - want).abs().max().item() if want.numel() else 0.0
    assert err <= atol + rtol * scale, '{}: max err {:.3e} against scale {:.3e}'.format(name, err, scale)


@contextlib.contextmanager
def _env(name, value):
    """os.environ[name] = value inside the block; the caller's value (or its absence) after it."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _zero_rows(t, rows, name):
    sel = t[rows]
    assert sel.numel() == 0 or (sel == 0).all().item(), name + ': rows that must be exactly 0 are not'


# ---------------------------------------------------------------------------------------------------
# grouped GEMMs

def _ref_grouped(a, w, sizes, n, k, gather=None, bias=None, scale=None):
    """fp64 out[p] = scale[p] * (a[gather[p]] @ W_g^T + bias[g]) for W = w.view(G, n, k)."""
    a, w = a.double().cpu(), w.double().cpu().view(len(sizes), n, k)
    rows = torch.arange(sum(sizes)) if gather is None else gather.long().cpu()
    out = torch.zeros([sum(sizes), n], dtype=torch.float64)
    lo = 0
    for g, m in enumerate(sizes):
        o = a[rows[lo:lo + m]] @ w[g].T
        if bias is not None:
            o = o + bias.double().cpu()[g]
        if scale is not None:
            o = o * scale.double().cpu()[lo:lo + m, None]
        out[lo:lo + m] = o
        lo += m
    return out


GG_SIZES = [0, 1, 0, 150, 0]          # first, middle and last group empty; a 1-row group


def _gg_fp32():
    from naive_gpt import ext
    gen = _gen(1)
    G, n, k, T = len(GG_SIZES), 200, 72, 190          # N % 128 and K % 32 tails
    P = sum(GG_SIZES)
    a, w, bias = _randn(gen, T, k), _randn(gen, G * n, k), _randn(gen, G, n)
    gather = _dev(torch.randint(0, T, [P], generator=gen, dtype=torch.int32))
    scale = _dev(torch.rand([P], generator=gen) + 0.5)
    off = _offsets(GG_SIZES)

    def call():
        return ext.grouped_gemm(a, w, off, G, n, k, n * k, k, 1, gather=gather, bias=bias, rowscale=scale)

    def check(outs):
        _close(outs[0], _ref_grouped(a, w, GG_SIZES, n, k, gather, bias, scale), 'out')
    return call, check


KINK_SIZES = [0, 200, 0, 312, 0]      # empty first, middle and last groups


def _near_kink_operands(gen, K, N):
    """a [P, K], w [G * N, K] whose pre-activations (g, n) . (lo_g + n) sit 1e-7 .. 1e-4 from zero
    (each weight row made orthogonal to one row of a, then nudged), as
    test_relu_preactivations_near_the_kink_are_fp32_exact builds them: the ReLU-fix queue decides
    their signs."""
    G, P = len(KINK_SIZES), sum(KINK_SIZES)
    offsets = np.concatenate([[0], np.cumsum(KINK_SIZES)])
    a = torch.randn([P, K], generator=gen, dtype=torch.float64)
    w = torch.randn([G * N, K], generator=gen, dtype=torch.float64)
    nudge = torch.randn([G * N], generator=gen, dtype=torch.float64) * 10.0 ** (
        -4.0 - 3.0 * torch.rand([G * N], generator=gen, dtype=torch.float64))
    for g in range(G):
        for n in range(min(N, KINK_SIZES[g])):
            row, p = g * N + n, offsets[g] + n
            w[row] -= (w[row] @ a[p] - nudge[row]) / (a[p] @ a[p]) * a[p]
    return _dev(a.float()), _dev(w.float())


def _gg_fused(images):
    def build():
        from naive_gpt import ext
        G, n, k = len(KINK_SIZES), 256, 256
        P = sum(KINK_SIZES)
        a, w = _near_kink_operands(_gen(31), k, n)
        off = _offsets(KINK_SIZES)

        def call():
            kw = {'w_image': ext.split_bf16(w)}
            if images == 'image':
                kw['a_image'] = ext.split_bf16(a)
            h, pre = ext.grouped_gemm_fused(a, w, off, G, n=n, k=k, w_group_stride=n * k, w_ldn=k, w_ldk=1,
                                            n_rows=P, epilogue=ext.EPI_ACT, activation=ext.ACT_RELU,
                                            keep_preact=True, **kw)
            assert ext.LAST_GEMM_PATH == images
            # the queue's per-segment counters (gg_epilogue of grouped_gemm.h, one every 16 words)
            counts = ext.LAST_RELU_QUEUE[:256 * 64].view(torch.int32).view(256, 16)[:, 0].clone()
            return h, pre, counts

        def check(outs):
            h, pre, counts = outs
            want = _ref_grouped(a, w, KINK_SIZES, n, k)
            _close(pre, want, 'preact', rtol=1e-5)
            assert int(counts.sum()) >= 300, 'ReLU-fix queue holds {} entries'.format(int(counts.sum()))
            assert torch.equal(h, pre.clamp_min(0.0))
            an, wn = a.double().norm(dim=1).cpu(), w.double().norm(dim=1).cpu().view(G, n)
            bound = torch.cat([an[lo:lo + m, None] * wn[g][None, :]
                               for g, lo, m in zip(range(G), np.cumsum([0] + KINK_SIZES), KINK_SIZES)])
            decided = want.abs() > 3e-7 * bound          # beyond the fp32 recomputation's error
            assert ((pre.double().cpu() > 0) == (want > 0))[decided].all(), 'a ReLU sign differs from fp64'
        return call, check
    return build


def _gg_dact():
    """EPI_DACT: out = v * relu'(s) and the per-column-tile row dots <v, h>, <out, h> (raw_dots: the
    [P, pdot_width] buffers themselves), v = a[gather] W_g^T + a2 b2_g^T."""
    from naive_gpt import ext
    gen = _gen(33)
    G, n, k, r, T = len(GG_SIZES), 200, 64, 8, 120
    P = sum(GG_SIZES)
    a, w = _randn(gen, T, k), _randn(gen, G * n, k)
    a2, b2 = _randn(gen, T, r), _randn(gen, G * n, r)
    gather = _dev(torch.randint(0, T, [P], generator=gen, dtype=torch.int32))
    h = _dev(torch.relu(_randn(gen, P, n)))
    off = _offsets(GG_SIZES)

    def call():
        return ext.grouped_gemm_fused(a, w, off, G, n=n, k=k, w_group_stride=n * k, w_ldn=k, w_ldk=1, n_rows=P,
                                      gather=gather, a2=a2, gather2=gather, b2=b2, b2_group_stride=n * r,
                                      epilogue=ext.EPI_DACT, activation=ext.ACT_RELU, h_in=h, raw_dots=True)

    def check(outs):
        out, dot_main, dot_act = outs
        v = _ref_grouped(a, w, GG_SIZES, n, k, gather) + _ref_grouped(a2, b2, GG_SIZES, n, r, gather)
        want = v * (h.double().cpu() > 0)
        _close(out, want, 'out')
        assert dot_main.shape == (P, ext.load_library().spt_grouped_gemm_pdot_width(n))
        _close(dot_main.sum(-1), (v * h.double().cpu()).sum(-1), 'dot_main', rtol=1e-4)
        _close(dot_act.sum(-1), (want * h.double().cpu()).sum(-1), 'dot_act', rtol=1e-4)
    return call, check


def _gg_bf16():
    from naive_gpt import ext
    gen = _gen(3)
    G, n, k = len(GG_SIZES), 96, 64
    P = sum(GG_SIZES)
    a, w = _randn(gen, P, k, dtype=torch.bfloat16), _randn(gen, G * n, k, dtype=torch.bfloat16)
    off = _offsets(GG_SIZES)

    def call():
        return ext.grouped_gemm_bf16(a, w, off, G, n, k, n * k, k, 1, n_rows=P)

    def check(outs):
        _close(outs[0], _ref_grouped(a, w, GG_SIZES, n, k), 'out', rtol=1e-2)
    return call, check


def _gg_bf16_ext():
    from naive_gpt import ext
    gen = _gen(4)
    G, n, k, r = len(GG_SIZES), 96, 64, 16
    P = sum(GG_SIZES)
    a, w = _randn(gen, P, k, dtype=torch.bfloat16), _randn(gen, G * n, k, dtype=torch.bfloat16)
    a2, b2 = _randn(gen, P, r), _randn(gen, G * n, r, dtype=torch.bfloat16)
    off = _offsets(GG_SIZES)

    def call():
        return ext.grouped_gemm_bf16_ext(a, w, off, G, n, k, n * k, k, 1, a2, b2, n * r, n_rows=P)

    def check(outs):
        want = _ref_grouped(a, w, GG_SIZES, n, k) + _ref_grouped(a2, b2, GG_SIZES, n, r)
        _close(outs[0], want, 'out', rtol=1e-2)
    return call, check


def _wgrad(dtype, gathers):
    def build():
        from naive_gpt import ext
        from test_gpu_routed_train import ref_wgrad
        gen = _gen(5)
        sizes = [0, 37, 0, 1, 300, 0]
        P, G, T = sum(sizes), len(sizes), 400
        n, k = 100, 72
        view, size = (n, k, n * k, k, 1), G * n * k
        grad = torch.randn([T if gathers else P, n], generator=gen)
        a = torch.randn([T if gathers else P, k], generator=gen)
        if dtype == torch.bfloat16:
            grad, a = grad.bfloat16(), a.bfloat16()
        gg = torch.randint(0, T, [P], generator=gen, dtype=torch.int32) if gathers else None
        ga = torch.randint(0, T, [P], generator=gen, dtype=torch.int32) if gathers else None
        scale = torch.rand([P], generator=gen) + 0.5
        want, want_bias = ref_wgrad(grad.double(), a.double(), [0] + list(np.cumsum(sizes)), view, gg, ga,
                                    scale, size)
        args = [None if t is None else _dev(t) for t in (grad, a, gg, ga, scale)]
        off = _offsets(sizes)

        def call():
            return ext.grouped_gemm_wgrad(args[0], args[1], off, view, P, gather_grad=args[2], gather_a=args[3],
                                          rowscale=args[4], want_bias=True)

        def check(outs):
            rtol = 1e-2 if dtype == torch.bfloat16 else 1e-5
            _close(outs[0], want, 'dW', rtol=rtol)
            _close(outs[1], want_bias, 'dbias', rtol=rtol)
            dw = outs[0].view(G, n, k)
            for g, m in enumerate(sizes):
                if m == 0:
                    assert (dw[g] == 0).all() and (outs[1][g] == 0).all(), 'empty group %d not exactly 0' % g
        return call, check
    return build


def _split_bf16():
    from naive_gpt import ext
    gen = _gen(6)
    rows, cols, G, n = 33, 40, 1, 96            # cols % 32 != 0: 24 pad columns in the image
    x, w = _randn(gen, rows, cols), _randn(gen, G * n, cols)
    off = _offsets([rows])

    def call():
        img = ext.split_bf16(x)
        out = ext.grouped_gemm_fused(x, w, off, G, n=n, k=cols, w_group_stride=n * cols, w_ldn=cols, w_ldk=1,
                                     n_rows=rows, a_image=img, w_image=ext.split_bf16(w))
        return img.buffer, out

    def check(outs):
        blocks = (cols + 31) // 32
        raw = outs[0].view(torch.bfloat16).view(rows, blocks, 2, 32)
        pad = _dev(torch.zeros([rows, blocks * 32]))
        pad[:, :cols] = x
        hi = pad.bfloat16()
        lo = (pad - hi.float()).bfloat16()
        assert torch.equal(raw[:, :, 0].reshape(rows, -1).view(torch.int16), hi.view(torch.int16))
        assert torch.equal(raw[:, :, 1].reshape(rows, -1).view(torch.int16), lo.view(torch.int16))
        assert (raw.reshape(rows, blocks, 2 * 32)[:, -1].view(rows, 2, 32)[:, :, cols % 32:] == 0).all(), \
            'image pad columns past cols are not 0'
        _close(outs[1], _ref_grouped(x, w, [rows], n, cols), 'x @ W^T through the image', rtol=1e-5)
    return call, check


# ---------------------------------------------------------------------------------------------------
# tall_tn: wide^T . narrow per row group

TN_SIZES = ([0, 16384, 0, 0], [1, 63, 64, 65, 129, 0, 7, 5000])


def _ref_tall_tn(wide, narrow, sizes):
    wide, narrow = wide.double().cpu(), narrow.double().cpu()
    out, lo = [], 0
    for m in sizes:
        out.append(wide[lo:lo + m].T @ narrow[lo:lo + m])
        lo += m
    return torch.stack(out)


def _tall_tn(which, sizes):
    def build():
        from naive_gpt import ext
        gen = _gen(7 + len(sizes))
        rows, width, n = sum(sizes), 64, 16
        dt = torch.bfloat16 if which == 'bf16' else torch.float32
        wides = [_randn(gen, rows, width, dtype=dt) for _ in range(2)]
        narrows = [_randn(gen, rows, n) for _ in range(2)]
        off = _offsets(sizes)

        def call():
            if which == 'single':
                return ext.tall_tn(wides[0], narrows[0], offsets=off)
            if which == 'batch':
                return ext.tall_tn_batch(wides, narrows, offsets=off)
            return ext.tall_tn_bf16(wides[0], narrows[0], offsets=off)

        def check(outs):
            for i in range(2 if which == 'batch' else 1):
                want = _ref_tall_tn(wides[i], narrows[i], sizes)
                g = outs[i]
                _close(g, want, 'tall_tn', rtol=1e-2 if which == 'bf16' else 1e-5)
                for j, m in enumerate(sizes):
                    if m == 0:
                        assert (g[j] == 0).all(), 'empty group %d not exactly 0' % j
        return call, check
    return build


# ---------------------------------------------------------------------------------------------------
# lora_down family: u = x @ table, images and norms as by-products

def _lora_down():
    from naive_gpt import ext
    gen = _gen(8)
    rows, K, n = 1000, 96, 32                 # rows not a multiple of the row tile
    x, t = _randn(gen, rows, K), _randn(gen, K, n)

    def call():
        u, img, norms = ext.lora_down(x, t, want_image=True, want_norms=True)
        pack = ext.lora_down(x, t, block_major=True, exact=True)
        return u, img.buffer, norms, pack

    def check(outs):
        want = x.double() @ t.double()
        _close(outs[0], want, 'u', rtol=1e-5)
        _close(outs[2], x.double().norm(dim=1), 'norms', rtol=1e-6)
        _close(outs[3], want.view(rows, n // 16, 16).transpose(0, 1), 'u block-major exact', rtol=1e-6)
        assert torch.equal(outs[1], ext.split_bf16(x).buffer), 'by-product image differs from split_bf16'
    return call, check


def _lora_down_table2():
    """spt_lora_down2: a second, row-major table [n2, K] as the last 16-column block, whose columns
    n2 .. 15 are written as 0 (lora_side.hip:101)."""
    from naive_gpt import ext
    gen = _gen(34)
    rows, K, n, n2 = 1000, 96, 32, 5
    x, t, t2 = _randn(gen, rows, K), _randn(gen, K, n), _randn(gen, n2, K) / 16

    def call():
        return ext.lora_down(x, t, block_major=True, exact=True, table2=t2)

    def check(outs):
        pack = outs[0]
        assert pack.shape == (n // 16 + 1, rows, 16)
        _close(pack[:-1], (x.double() @ t.double()).view(rows, n // 16, 16).transpose(0, 1), 'u', rtol=1e-6)
        _close(pack[-1][:, :n2], x.double() @ t2.double().T, 'x . table2^T', rtol=1e-6)
        assert (pack[-1][:, n2:] == 0).all(), 'columns n2 .. 15 of the table2 block are not exactly 0'
    return call, check


def _lora_down_tables():
    from naive_gpt import ext
    gen = _gen(9)
    rows, K = 777, 64
    x, stack = _randn(gen, rows, K), _randn(gen, 3, K, 16)
    tables = list(stack.unbind(0))

    def call():
        u, img = ext.lora_down_tables(x, tables, want_image=True)
        return u, img.buffer

    def check(outs):
        _close(outs[0], torch.stack([x.double() @ t.double() for t in tables]), 'u', rtol=1e-5)
        assert torch.equal(outs[1], ext.split_bf16(x).buffer)
    return call, check


def _lora_down_stacked():
    from naive_gpt import ext
    gen = _gen(10)
    G, rows, K = 3, 333, 64
    xs, stack = _randn(gen, G, rows, K), _randn(gen, G, K, 16)
    off = _dev(torch.arange(0, G * rows + 1, rows, dtype=torch.int32))

    def call():
        out = torch.empty([rows, 16 * G], device=xs.device)
        return ext.lora_down_stacked(list(xs.unbind(0)), list(stack.unbind(0)), off, out)

    def check(outs):
        want = torch.cat([xs[g].double() @ stack[g].double() for g in range(G)], 1)
        _close(outs[0], want, 'out', rtol=1e-5)
    return call, check


def _lora_down_grouped(bf16):
    def build():
        from naive_gpt import ext
        gen = _gen(11)
        sizes, K, n = [0, 300, 0, 1, 200, 0], 64, 16
        rows, G = sum(sizes), len(sizes)
        dt = torch.bfloat16 if bf16 else torch.float32
        x, tables = _randn(gen, rows, K, dtype=dt), _randn(gen, G, K, n, dtype=dt)
        off = _offsets(sizes)

        def call():
            if bf16:
                return ext.lora_down_grouped_bf16(x, tables, off)
            u, img = ext.lora_down_grouped(x, tables, off, want_image=True)
            return u, img.buffer

        def check(outs):
            want, lo = torch.zeros([rows, n], dtype=torch.float64), 0
            for g, m in enumerate(sizes):
                want[lo:lo + m] = x[lo:lo + m].double().cpu() @ tables[g].double().cpu()
                lo += m
            _close(outs[0], want, 'u', rtol=1e-5)
            if not bf16:
                assert torch.equal(outs[1], ext.split_bf16(x).buffer)
        return call, check
    return build


def _lora_down_bf16():
    from naive_gpt import ext
    gen = _gen(12)
    rows, K, n = 1000, 128, 32
    x, t = _randn(gen, rows, K, dtype=torch.bfloat16), _randn(gen, K, n, dtype=torch.bfloat16)

    def call():
        return ext.lora_down_bf16(x, t), ext.lora_down_bf16(x, t, block_major=True)

    def check(outs):
        want = x.double() @ t.double()
        _close(outs[0], want, 'u', rtol=1e-5)
        _close(outs[1], want.view(rows, n // 16, 16).transpose(0, 1), 'u block-major', rtol=1e-5)
    return call, check


# ---------------------------------------------------------------------------------------------------
# routing: every token to the same two blocks, the other groups empty; T not a multiple of 256

R_T, R_G, R_K, R_SCALE = 300, 8, 2, 2.0


def _route_prob(gen):
    """Two blocks that the seed picks take every token: never the first or the last, and one block
    apart (empty groups at both ends and between them).  Another seed gives another routing of the
    same shape."""
    prob = torch.rand([R_T, R_G], generator=gen) * 0.5
    lo = 1 + int(torch.randint(0, R_G - 4, [1], generator=gen))
    hi = lo + 2
    prob[:, lo] += 0.6
    prob[:, hi] += 0.55
    return _dev(prob)


def _hot_blocks(prob):
    """The two blocks _route_prob raised (>= 0.55 against < 0.5 everywhere else), in order."""
    hot = sorted(prob[0].topk(2).indices.tolist())
    assert (prob[:, hot] > 0.525).all() and (prob > 0.525).sum().item() == 2 * R_T
    return hot


def _check_routing(prob, token, block, offsets, pos):
    lo, hi = _hot_blocks(prob)
    assert offsets.tolist() == [0] * (lo + 1) + [R_T] * (hi - lo) + [2 * R_T] * (R_G - hi)
    assert block.tolist() == [lo] * R_T + [hi] * R_T
    assert sorted(token[:R_T].tolist()) == list(range(R_T)) and sorted(token[R_T:].tolist()) == list(range(R_T))
    p = pos.long()
    assert (token[p] == _dev(torch.arange(R_T))[:, None]).all()


def _route_topk():
    from naive_gpt import ext
    prob = _route_prob(_gen(13))

    def call():
        return ext.route_topk(prob, R_K)

    def check(outs):
        _check_routing(prob, *outs)
    return call, check


def _route_topk_coeff():
    from naive_gpt import ext
    prob = _route_prob(_gen(14))

    def call():
        return ext.route_topk_coeff(prob, R_K, R_SCALE)

    def check(outs):
        token, block, offsets, pos, t64, b64, coeff = outs
        _check_routing(prob, token, block, offsets, pos)
        assert torch.equal(t64, token.long()) and torch.equal(b64, block.long())
        assert torch.equal(coeff, R_SCALE * prob[token.long(), block.long()])
    return call, check


def _route_topk_logits():
    from naive_gpt import ext
    gen = _gen(15)
    prob = _route_prob(gen).clamp(1e-3, 1 - 1e-3)
    bias = _dev(torch.rand([R_G], generator=gen) * 0.01)
    logits = _dev(torch.zeros([R_T, 16]))
    logits[:, :R_G] = torch.log(prob / (1 - prob)) - bias

    def call():
        return ext.route_topk_logits(logits, bias, R_G, R_K, R_SCALE)

    def check(outs):
        p, token, block, offsets, pos, t64, b64, coeff = outs
        want = torch.sigmoid(logits[:, :R_G].double() + bias.double())
        _close(p, want, 'prob', rtol=1e-6)
        _check_routing(want, token, block, offsets, pos)        # (the hot blocks from the reference, not from p)
        assert torch.equal(coeff, R_SCALE * p[token.long(), block.long()])
    return call, check


def _route_coeff_backward(with_prob):
    def build():
        from naive_gpt import ext
        gen = _gen(16)
        prob = _route_prob(gen)
        token, block, offsets, pos = ext.route_topk(prob, R_K)
        dcoeff = _randn(gen, R_T * R_K)
        sig = _dev(torch.sigmoid(prob))

        def call():
            return ext.route_coeff_backward(dcoeff, pos, block, R_SCALE, R_G, prob=sig if with_prob else None)

        def check(outs):
            want = _dev(torch.zeros([R_T, R_G], dtype=torch.float64))
            want[token.long(), block.long()] = R_SCALE * dcoeff.double()
            if with_prob:
                want = want * sig.double() * (1 - sig.double())
            _close(outs[0], want, 'dprob', rtol=1e-6)
            cold = [g for g in range(R_G) if g not in _hot_blocks(prob)]
            assert len(cold) == R_G - 2 and (outs[0][:, cold] == 0).all(), 'blocks no token picks: not exactly 0'
        return call, check
    return build


def _ffn_coeff_grad():
    from naive_gpt import ext
    gen = _gen(17)
    P, T, r, w = 301, 200, 16, 3
    dm, da, du, z = _randn(gen, P, w), _randn(gen, P, w), _randn(gen, P, r), _randn(gen, P, r)
    u, dzt = _randn(gen, T, r), _randn(gen, T, r)
    token = _dev(torch.randint(0, T, [P], generator=gen, dtype=torch.int32))
    coeff = _dev(torch.rand([P], generator=gen))

    def call():
        return ext.ffn_coeff_grad(dm, da, du, u, dzt, z, token, coeff, 0.25)

    def check(outs):
        t = token.long()
        d = lambda x: x.double()                # noqa: E731
        num = d(dm).sum(1) + d(da).sum(1) - (d(du) * d(u)[t]).sum(1) - (d(dzt)[t] * d(z)).sum(1)
        _close(outs[0], num / d(coeff).clamp(min=0.25), 'coeff grad', rtol=1e-5)
    return call, check


# ---------------------------------------------------------------------------------------------------
# row-wise kernels

def _rows_combine(form):
    def build():
        from naive_gpt import ext
        gen = _gen(18)
        T, k, d, ns = 257, 2, 100, 16
        dt = torch.bfloat16 if form == 'bf16' else torch.float32
        rows, bias = _randn(gen, T * k + 3, d, dtype=dt), _randn(gen, d, dtype=dt)
        pos = _dev(torch.randperm(T * k, generator=gen).int().view(T, k))
        side, sw = _randn(gen, T, ns), _randn(gen, ns, d)

        def call():
            if form == 'side':
                return ext.rows_combine(rows, pos, bias=bias, side=side, side_weight=sw)
            return ext.rows_combine(rows, pos, bias=bias)

        def check(outs):
            want = bias.double() + rows.double()[pos.long()].sum(1)
            if form == 'side':
                want = want + side.double() @ sw.double()
            _close(outs[0], want, 'out', rtol=1e-2 if form == 'bf16' else 1e-5)
        return call, check
    return build


def _swiglu(form):
    def build():
        from naive_gpt import ext
        gen = _gen(19)
        rows, n = 33, 100
        dt = torch.bfloat16 if form.endswith('bf16') else torch.float32
        g, s, dh = (_randn(gen, rows, n, dtype=dt) for _ in range(3))
        g64, s64 = g.double().requires_grad_(True), s.double().requires_grad_(True)
        h64 = torch.nn.functional.silu(g64) * s64
        dg64, ds64 = torch.autograd.grad(h64, (g64, s64), dh.double())

        def call():
            return {'fwd': lambda: ext.swiglu_forward(g, s), 'fwd_bf16': lambda: ext.swiglu_forward_bf16(g, s),
                    'bwd': lambda: ext.swiglu_backward(dh, g, s), 'bwd_bf16': lambda: ext.swiglu_backward_bf16(dh, g, s),
                    'dots_bf16': lambda: ext.swiglu_backward_dots_bf16(dh, g, s)}[form]()

        def check(outs):
            rtol = 1e-2 if dt == torch.bfloat16 else 1e-5
            if form.startswith('fwd'):
                _close(outs[0], h64, 'h', rtol=rtol)
                return
            _close(outs[0], dg64, 'dg', rtol=rtol)
            _close(outs[1], ds64, 'ds', rtol=rtol)
            if len(outs) > 2:
                h = h64.detach()
                dgs, dss = outs[0].double(), outs[1].double()
                _close(outs[2], (dh.double() * h).sum(1), 'dot_h', rtol=rtol)
                _close(outs[3], (dgs * g.double()).sum(1), 'dot_g', rtol=rtol)
                _close(outs[4], (dss * s.double()).sum(1), 'dot_s', rtol=rtol)
        return call, check
    return build


def _embedding_rows_backward():
    from naive_gpt import ext
    gen = _gen(20)
    rows, T, width = 50, 40, 24
    ids = _dev(torch.tensor([3, 7, 11, 49])[torch.randint(0, 4, [T], generator=gen)])
    g = _randn(gen, T, width)

    def call():
        return ext.embedding_rows_backward(g, ids, rows)

    def check(outs):
        want = _dev(torch.zeros([rows, width], dtype=torch.float64)).index_add_(0, ids, g.double())
        _close(outs[0], want, 'grad', rtol=1e-6)
        absent = _dev(torch.ones(rows, dtype=torch.bool))
        absent[ids] = False
        _zero_rows(outs[0], absent, 'rows no id names')
    return call, check


def _cross_entropy():
    from naive_gpt import ext
    gen = _gen(21)
    rows, V, ld = 33, 1001, 1008                  # V not a multiple of the block, pad columns
    z = _dev(3.0 * torch.randn([rows, V], generator=gen))
    target = _dev(torch.randint(0, V, [rows], generator=gen))
    target[::4] = -100
    buf0 = _dev(torch.full([rows, ld], 7.0))
    buf0[:, :V] = z
    scale = _dev((1.0 / (target != -100).sum().float()).reshape(1))

    def call():
        buf = _dev(buf0.clone())            # the entry works in place: its output is this operand
        loss = ext.cross_entropy_grad_(buf, V, target, scale)
        return loss, buf

    def check(outs):
        loss, buf = outs
        zr = z.double().requires_grad_(True)
        want = torch.nn.functional.cross_entropy(zr, target, reduction='none')
        want.sum().backward()
        _close(loss, want.detach(), 'loss rows', rtol=1e-5)
        assert (loss[::4] == 0).all() and (buf[::4] == 0).all(), 'ignored rows not exactly 0'
        _close(buf[:, :V], zr.grad * scale.double(), 'grad', rtol=1e-5)
        assert (buf[:, V:] == 0).all()
    return call, check


def _layernorm(rows, rms, width=None):
    def build():
        from naive_gpt import ext
        gen = _gen(22 + rows)
        d = min(ext.LAYERNORM_WIDTHS) if width is None else width
        x, r, dy, dskip = (_randn(gen, rows, d) for _ in range(4))
        gamma = _randn(gen, d)
        beta = None if rms else _randn(gen, d)

        def call():
            s, y, mean, rstd = ext.add_layernorm_forward(x, r, gamma, beta, 1e-5, rms=rms)
            dx, dgamma, dbeta = ext.layernorm_backward(s, dy, gamma, mean, rstd, dskip=dskip, rms=rms)
            return s, y, mean, rstd, dx, dgamma, dbeta

        def check(outs):
            s = (x.double() + r.double()).requires_grad_(True)
            g64 = gamma.double().requires_grad_(True)
            b64 = None if rms else beta.double().requires_grad_(True)
            if rms:
                y = s * torch.rsqrt(s.square().mean(-1, keepdim=True) + 1e-5) * g64
            else:
                y = torch.nn.functional.layer_norm(s, [d], g64, b64, 1e-5)
            y.backward(dy.double())
            _close(outs[0], s.detach(), 's', rtol=1e-6)
            _close(outs[1], y.detach(), 'y', rtol=1e-4)
            _close(outs[4], s.grad + dskip.double(), 'dx', rtol=1e-4)
            _close(outs[5], g64.grad, 'dgamma', rtol=1e-4)
            if rms:
                assert (outs[6] == 0).all(), 'rms: dbeta not exactly 0'
            else:
                _close(outs[6], b64.grad, 'dbeta', rtol=1e-4)
        return call, check
    return build


def _rotary(transpose):
    def build():
        from naive_gpt import ext, layers
        gen = _gen(23)
        N, S, H, E = 1, 130, 3, 64
        emb = layers.RotaryEmbedding(n_embeddings=256, d_model=E)._apply(_dev)      # its tables, as Module.cuda moves them
        xs = [_randn(gen, N, S, H, E) for _ in range(3)]
        ids = _dev(torch.arange(S))

        def call():
            return ext.rotary(xs, 2, emb.cos_cached, emb.sin_cached, transpose=transpose)

        def check(outs):
            out = outs[0]
            for p in range(3):
                if p >= 2:
                    want = xs[p]
                elif not transpose:
                    want = emb(xs[p], ids)
                else:           # the adjoint: <rot(a), b> == <a, rot^T(b)>
                    probe = _randn(gen, N, S, H, E)
                    lhs = (emb(probe, ids).double() * xs[p].double()).sum()
                    rhs = (probe.double() * out[p].double()).sum()
                    assert abs(lhs - rhs) <= 1e-4 * abs(lhs) + 1e-3
                    continue
                _close(out[p], want, 'part %d' % p, rtol=1e-6)
        return call, check
    return build


# ---------------------------------------------------------------------------------------------------
# PQ: cdist, codes, fused loss

def _cdist():
    from naive_gpt import ext
    from oracle import ext_stub
    gen = _gen(24)
    M, NQ, C, D = 4, 300, 32, 8
    q, t = torch.randn([M, NQ, D], generator=gen), torch.randn([M, C, D], generator=gen)
    go = torch.randn([M, NQ, C], generator=gen)
    go[:, :, 5:9] = 0                       # centroids whose distances get no gradient
    qd, td, god = _dev(q), _dev(t), _dev(go)

    def call():
        d, i = ext.cdist_forward_cuda(qd, td)
        return d, i, ext.cdist_encode(qd, td)

    def check(outs):
        d, i = ext_stub.cdist_forward_cuda(q, t)
        _close(outs[0], d, 'distance', rtol=1e-5)
        assert torch.equal(outs[1].cpu(), i) and torch.equal(outs[2].cpu(), i)
    return call, check, (q, t, go, qd, td, god)


def _cdist_fwd():
    call, check, _ = _cdist()
    return call, check


def _cdist_bwd():
    from naive_gpt import ext
    from oracle import ext_stub
    _, _, (q, t, go, qd, td, god) = _cdist()

    def call():
        return ext.cdist_backward_cuda(qd, td, god)

    def check(outs):
        wq, wt = ext_stub.cdist_backward_cuda(q, t, go)
        _close(outs[0], wq, 'grad_query', rtol=1e-5)
        _close(outs[1], wt, 'grad_table', rtol=1e-5)
        assert (outs[1][:, 5:9] == 0).all(), 'centroids without gradient: not exactly 0'
    return call, check


def _pq(which):
    def build():
        from naive_gpt import ext
        from oracle import ext_stub
        from test_gpu_pq_loss import composed_cpu
        gen = _gen(25)
        N, S, H, E, C = 1, 96, 4, 64, 16
        M, D = E // 8, 8
        z = torch.randn([N, S, H, E], generator=gen)
        k2 = torch.randn([N, S, H, E], generator=gen)
        table = torch.randn([M, C, D], generator=gen)
        zd, td = _dev(z), _dev(table)
        pair = _dev(torch.stack([z, k2]))
        upstream = _dev(torch.ones([]))
        assert ext.pq_loss_supported(zd, td)

        def call():
            if which == 'codes':
                return (ext.pq_encode_heads(zd, td),)
            if which == 'single':
                loss, codes = ext.pq_loss_forward(zd, td, want_codes=True)
                gz, gt = ext.pq_loss_backward(zd, td, upstream)
                return loss, codes, gz, gt
            loss, cq, ck = ext.pq_loss_forward_pair(pair[0], pair[1], td)
            both = _dev(torch.zeros([2, *z.shape]))
            gt = ext.pq_loss_backward_pair(pair[0], pair[1], td, upstream, both[0], both[1])
            return loss, cq, ck, both, gt

        def check(outs):
            flat = z.permute(0, 2, 1, 3).reshape(N * H * S, M, D).transpose(0, 1).contiguous()
            codes = ext_stub.cdist_forward_cuda(flat, table)[1].T.reshape(N * H, S, M)
            if which == 'codes':
                assert torch.equal(outs[0].cpu(), codes)
                return
            if which == 'single':
                loss, gz, gt = composed_cpu(z, table, 1.0)
                _close(outs[0], loss, 'loss', rtol=1e-3)
                assert torch.equal(outs[1].cpu(), codes)
                _close(outs[2], gz, 'grad_z', rtol=1e-3)
                _close(outs[3], gt, 'grad_table', rtol=1e-3)
            else:
                lq, gzq, gtq = composed_cpu(z, table, 1.0)
                lk, gzk, gtk = composed_cpu(k2, table, 1.0)
                _close(outs[0], lq + lk, 'loss', rtol=1e-3)
                assert torch.equal(outs[1].cpu(), codes)
                _close(outs[3][0], gzq, 'grad_q', rtol=1e-3)
                _close(outs[3][1], gzk, 'grad_k', rtol=1e-3)
                _close(outs[4], gtq + gtk, 'grad_table', rtol=1e-3)
        return call, check
    return build


def _lookup():
    from naive_gpt import ext
    from oracle import oracle as O
    gen = _gen(26)
    B, coeff, M = 1, 8, 8
    S = 256 * coeff                               # Z = 256; rows < Z are short: padded with column 0
    q = torch.randint(0, 3, [B, S, M], generator=gen, dtype=torch.int32)
    k = torch.randint(0, 3, [B, S, M], generator=gen, dtype=torch.int32)
    config = torch.empty([coeff], device='cpu')
    qd, kd = _dev(q), _dev(k)

    def call():
        return ext.lookup_forward_cuda(config, qd, kd)

    def check(outs):
        want = torch.from_numpy(np.asarray(O.lookup_forward(q.numpy(), k.numpy(), coeff)))
        assert torch.equal(outs[0].cpu().view(want.shape), want)
        assert (outs[0].view(B, S, 256)[:, 0, 1:] == 0).all(), 'short row 0: padding is not column 0'
    return call, check


# ---------------------------------------------------------------------------------------------------
# CSR kernels: sddmm, spmm (gather and matrix-core forms), softmax, transposes

def _csr_inputs(seed, B=3, S=100, E=64, max_row=12):
    from helpers import ragged_csr
    rng = np.random.default_rng(seed)
    indptr, idx = ragged_csr(rng, B, S, max_row)
    idx[:, :4] = idx[:, 0:1]                      # duplicate columns in the first row that has them
    indptr, idx = torch.from_numpy(indptr), torch.from_numpy(idx)
    gen = _gen(seed)
    q, k = torch.randn([B, S, E], generator=gen), torch.randn([B, S, E], generator=gen)
    vals = torch.randn([B, idx.size(1)], generator=gen)
    return indptr, idx, q, k, vals


def _sddmm():
    from naive_gpt import ext
    from oracle import ext_stub
    indptr, idx, q, k, _ = _csr_inputs(27)
    d = [_dev(t) for t in (indptr, idx, q, k)]

    def call():
        return ext.sddmm_forward_cuda(False, True, *d, scale=0.5, clamp=3.0)

    def check(outs):
        f, t = torch.scalar_tensor(False), torch.scalar_tensor(True)
        want = (ext_stub.sddmm_forward_cuda(f, t, indptr, idx, q, k) * np.float32(0.5)).clamp(-3.0, 3.0)
        _close(outs[0], want, 'scores', rtol=1e-5)
    return call, check


def _spmm(trans, mfma):
    def build():
        from naive_gpt import ext
        from oracle import ext_stub
        if mfma:            # the matrix-core form takes uniform rows of at least S / 16 entries
            from helpers import uniform_csr
            rng = np.random.default_rng(28 + trans)
            indptr, idx = (torch.from_numpy(t) for t in uniform_csr(rng, 2, 256, 32, True))
            gen = _gen(28)
            x, vals = torch.randn([2, 256, 64], generator=gen), torch.randn([2, idx.size(1)], generator=gen)
        else:
            indptr, idx, _, x, vals = _csr_inputs(28 + trans)
        d = [_dev(t) for t in (indptr, idx, vals, x)]

        def call():
            with _env('SPT_SPMM_MFMA', '1' if mfma else '0'):
                return ext.spmm_forward_cuda(trans, False, *d)

        def check(outs):
            want = ext_stub.spmm_forward_cuda(torch.scalar_tensor(trans), torch.scalar_tensor(False),
                                              indptr, idx, vals, x)
            _close(outs[0], want, 'y', rtol=1e-5)
            if not trans and not mfma:
                empty = _dev(indptr[1:] == indptr[:-1])
                assert empty.any()
                assert (outs[0][:, empty] == 0).all(), 'empty rows not exactly 0'
        return call, check
    return build


def _spmm_transposed(memo):
    def build():
        from naive_gpt import ext
        from oracle import ext_stub
        indptr, idx, _, x, vals = _csr_inputs(30)
        d_indptr, d_idx, d_vals, d_x = [_dev(t) for t in (indptr, idx, vals, x)]

        def call():
            t = ext.transposed_for(d_indptr, d_idx) if memo else ext.csr_transpose(d_indptr, d_idx)
            return ext.spmm_transposed(t, d_indptr, d_idx, d_vals, d_x)

        def check(outs):
            want = ext_stub.spmm_forward_cuda(torch.scalar_tensor(True), torch.scalar_tensor(False),
                                              indptr, idx, vals, x)
            _close(outs[0], want, 'y', rtol=1e-5)
        return call, check, (d_idx,)
    return build


def _softmax(which):
    def build():
        from naive_gpt import ext
        from oracle import ext_stub
        indptr, idx, _, _, vals = _csr_inputs(31)
        gen = _gen(31)
        dy = torch.randn(vals.shape, generator=gen)
        y = ext_stub.softmax_forward_cuda(indptr, idx, vals)
        raw = vals * 4.0
        scores = (raw * np.float32(0.5)).clamp(-1.0, 1.0)
        d = _dev

        def call():
            if which == 'fwd':
                return ext.softmax_forward_cuda(d(indptr), d(idx), d(vals))
            if which == 'bwd':
                return ext.softmax_backward_cuda(d(indptr), d(idx), d(y), d(dy))
            return ext.softmax_backward_clamped(d(indptr), d(idx), d(y), d(dy), d(scores), 0.5, 1.0)

        def check(outs):
            if which == 'fwd':
                want = y
            else:
                want = ext_stub.softmax_backward_cuda(indptr, idx, y, dy)
                if which == 'clamped':
                    want = torch.where(scores.abs() < 1.0, want * np.float32(0.5), torch.zeros_like(want))
            _close(outs[0], want, which, rtol=1e-5)
        return call, check
    return build


# ---------------------------------------------------------------------------------------------------
# attention

CLAMP = 10.0


def _dead_key_indices(B, S, Z, gen, distinct=False):
    """Causal uniform rows whose columns stay below S // 2: keys S // 2 .. S - 1 are attended by
    no query, so their grad_k and grad_v rows are exactly 0.  `distinct`: as lookup emits rows
    (distinct columns, then padding with column 0), which the compact tiles require."""
    idx = torch.zeros([B, S, Z], dtype=torch.int32)
    for r in range(S):
        hi = min(r, S // 2 - 1) + 1
        n = min(r + 1, Z)
        if not distinct:
            idx[:, r, :n] = torch.randint(0, hi, [B, n], generator=gen, dtype=torch.int32)
            continue
        for b in range(B):
            cols = torch.randperm(hi, generator=gen)[:n].int()
            idx[b, r, :cols.numel()] = cols
    return idx.view(B, S * Z)


def _once(memo, make):
    """make(), computed by the first build of a case and shared by its later ones: the inputs come
    from the case's seed, so every build would compute the same reference."""
    if 'value' not in memo:
        memo['value'] = make()
    return memo['value']


def _attn_refs(idx, q, k, v, gy, scale):
    from oracle import ext_stub
    from test_gpu_fused_attention import oracle_chain
    N, S, H, E = q.shape
    B = N * H
    scores, attn, y = oracle_chain(idx, q, k, v, scale)
    flat = lambda t: t.transpose(1, 2).contiguous().view(B, S, E)       # noqa: E731
    heads = lambda t: t.view(N, H, S, E).transpose(1, 2)                  # noqa: E731
    indptr = torch.arange(0, idx.size(1) + 1, idx.size(1) // S, dtype=torch.int32)
    f, t = torch.scalar_tensor(False), torch.scalar_tensor(True)
    dp = ext_stub.sddmm_forward_cuda(f, t, indptr, idx, gy, flat(v))
    ds = ext_stub.softmax_backward_cuda(indptr, idx, attn, dp)
    raw = torch.where(scores.abs() < CLAMP, ds * np.float32(scale), torch.zeros_like(ds))
    return (scores, attn, y, heads(ext_stub.spmm_forward_cuda(f, f, indptr, idx, raw, flat(k))),
            heads(ext_stub.spmm_forward_cuda(t, f, indptr, idx, raw, flat(q))),
            heads(ext_stub.spmm_forward_cuda(t, f, indptr, idx, attn, gy)), raw)


def _mfma(N, H, S, Z, E, gt, builder=None, bf16=False):
    memo = {}

    def build():
        from naive_gpt import ext
        gen = _gen(S + Z + E)
        B = N * H
        q, k, v = [torch.randn([N, S, H, E], generator=gen) for _ in range(3)]
        q = q * 3.0
        gy = torch.randn([B, S, E], generator=gen)
        if bf16:
            q, k, v, gy = (t.bfloat16().float() for t in (q, k, v, gy))
        idx = _dead_key_indices(B, S, Z, gen, distinct=builder is not None)
        scale = E ** -0.5
        dt = torch.bfloat16 if bf16 else torch.float32
        qd, kd, vd = (_dev(t.to(dt)) for t in (q, k, v))
        idd = _dev(idx)
        gyd = _dev((gy.transpose(1, 2).contiguous() if gt else gy).to(dt))
        refs = _once(memo, lambda: _attn_refs(idx, q, k, v, gy, scale))

        layout = {}

        def call():
            env = {'bits': 'SPT_CELL_TILES_BITS', 'counts': 'SPT_CELL_TILES_COUNTS'}.get(builder)
            with _env(env, '1') if env else contextlib.nullcontext():
                tiles = ext.attention_mfma_prepare(idd, S, lookup_pattern=builder is not None)
            layout['compact'], layout['tiles'] = tiles.layout == ext.TILES_COMPACT, tiles
            y, row_sum = ext.attention_mfma_forward(tiles, qd, kd, vd, scale, CLAMP, y_transposed=gt)
            gq, gk, gv = ext.attention_mfma_backward(tiles, qd, kd, vd, y, gyd, row_sum, scale, CLAMP,
                                                     transposed=gt)
            return y, row_sum, gq, gk, gv

        def check(outs):
            # (the promise flag is read here, after the call: a host read inside `call` would keep
            # the case from being captured in a HIP graph, tests/test_gpu_graph_replay.py)
            assert layout['compact'] == (builder is not None), 'tile layout: compact {}'.format(layout['compact'])
            assert not (layout['compact'] and layout['tiles'].broke_promise()), 'the compact tiles broke their promise'
            y, _, gq, gk, gv = outs
            if gt:
                y = y.transpose(1, 2)
            rtol = 2e-2 if bf16 else 1e-3
            _close(y, refs[2], 'y', rtol=rtol)
            for got, want, name in ((gq, refs[3], 'grad_q'), (gk, refs[4], 'grad_k'), (gv, refs[5], 'grad_v')):
                _close(got, want, name, rtol=rtol * 2)
            for got, name in ((gk, 'grad_k'), (gv, 'grad_v')):
                assert (got[:, S // 2:] == 0).all(), name + ': keys no query attends are not exactly 0'
        return call, check
    return build


def _fused_attention(S, yt, causal):
    memo = {}

    def build():
        from naive_gpt import ext
        from test_gpu_fused_attention import causal_indices
        N, H, Z, E = 1, 32, 16, 64                 # the fused kernels take B = N * H >= 32
        gen = _gen(S + 3)
        B = N * H
        q, k, v = [torch.randn([N, S, H, E], generator=gen) for _ in range(3)]
        gy = torch.randn([B, S, E], generator=gen)
        idx = causal_indices(B, S, Z, gen)
        scale = E ** -0.5
        refs = _once(memo, lambda: _attn_refs(idx, q, k, v, gy, scale))
        qd, kd, vd, idd = _dev(q), _dev(k), _dev(v), _dev(idx)
        gyd = _dev(gy.transpose(1, 2).contiguous() if yt else gy)
        assert ext.fused_attention_supported(S, E, B, S * Z)

        def call():
            scores, attn, y = ext.sparse_attention_forward(idd, qd, kd, vd, scale, CLAMP, y_transposed=yt,
                                                           causal=causal)
            graw, gq, rows = ext.sparse_attention_backward_rows(idd, gyd, vd, kd, scores, attn, scale, CLAMP,
                                                                grad_y_transposed=yt, causal=causal)
            return scores, attn, y, graw, gq, rows

        def check(outs):
            scores, attn, y, graw, gq, rows = outs
            _close(scores, refs[0], 'scores', rtol=1e-5)
            _close(attn, refs[1], 'attn', rtol=1e-4)
            _close(y.transpose(1, 2) if yt else y, refs[2], 'y', rtol=1e-4)
            _close(graw, refs[6], 'grad_raw', rtol=1e-4)
            _close(gq, refs[3], 'grad_q', rtol=1e-4)
            _close(rows, gy, 'grad_y rows', rtol=0)
        return call, check
    return build


# ---------------------------------------------------------------------------------------------------
# the registry: ext entry -> its cases

CASES = {
    'grouped_gemm': [Case('fp32_empty_groups_n_k_tails', _gg_fp32, DET)],
    'grouped_gemm_fused': [Case('relu_near_kink_image', _gg_fused('image'), DET),
                           Case('relu_near_kink_a32', _gg_fused('a32'), DET),
                           Case('dact_row_dots', _gg_dact, DET)],
    'grouped_gemm_bf16': [Case('empty_groups', _gg_bf16, DET)],
    'grouped_gemm_bf16_ext': [Case('empty_groups_lora_k_extension', _gg_bf16_ext, DET)],
    'grouped_gemm_wgrad': [Case('fp32_gathered', _wgrad(torch.float32, True), DET),
                           Case('fp32_plain', _wgrad(torch.float32, False), DET),
                           Case('bf16_gathered', _wgrad(torch.bfloat16, True), DET)],
    'split_bf16': [Case('cols_40_pad_and_gemm', _split_bf16, DET)],
    'tall_tn': [Case('sizes_%d' % i, _tall_tn('single', s), DET) for i, s in enumerate(TN_SIZES)],
    'tall_tn_batch': [Case('sizes_%d' % i, _tall_tn('batch', s), DET) for i, s in enumerate(TN_SIZES)],
    'tall_tn_bf16': [Case('sizes_%d' % i, _tall_tn('bf16', s), DET) for i, s in enumerate(TN_SIZES)],
    'lora_down': [Case('ragged_rows_image_norms_block_major', _lora_down, DET),
                  Case('table2_zero_columns', _lora_down_table2, DET)],
    'lora_down_tables': [Case('three_tables_image', _lora_down_tables, DET)],
    'lora_down_stacked': [Case('three_stacked', _lora_down_stacked, DET)],
    'lora_down_grouped': [Case('empty_groups_image', _lora_down_grouped(False), DET)],
    'lora_down_grouped_bf16': [Case('empty_groups', _lora_down_grouped(True), DET)],
    'lora_down_bf16': [Case('ragged_rows', _lora_down_bf16, DET)],
    'route_topk': [Case('two_blocks_take_all', _route_topk, DET)],
    'route_topk_coeff': [Case('two_blocks_take_all', _route_topk_coeff, DET)],
    'route_topk_logits': [Case('two_blocks_take_all', _route_topk_logits, DET)],
    'route_coeff_backward': [Case('dprob', _route_coeff_backward(False), DET),
                             Case('dlogit', _route_coeff_backward(True), DET)],
    'ffn_coeff_grad': [Case('ragged_rows', _ffn_coeff_grad, DET)],
    'rows_combine': [Case('fp32', _rows_combine('fp32'), DET), Case('bf16', _rows_combine('bf16'), DET),
                     Case('side', _rows_combine('side'), DET)],
    'swiglu_forward': [Case('ragged', _swiglu('fwd'), DET)],
    'swiglu_forward_bf16': [Case('ragged', _swiglu('fwd_bf16'), DET)],
    'swiglu_backward': [Case('ragged', _swiglu('bwd'), DET)],
    'swiglu_backward_bf16': [Case('ragged', _swiglu('bwd_bf16'), DET)],
    'swiglu_backward_dots_bf16': [Case('ragged', _swiglu('dots_bf16'), DET)],
    'embedding_rows_backward': [Case('four_ids_named', _embedding_rows_backward, DET)],
    'cross_entropy_grad_': [Case('ignored_rows_ragged_v', _cross_entropy, DET)],
    'add_layernorm_forward': [Case('rows_%d_%s' % (r, 'rms' if m else 'ln'), _layernorm(r, m), DET)
                              for r in (1, 37) for m in (False, True)],
    'layernorm_backward': [Case('rows_37_ln', _layernorm(37, False), DET)],
    'cdist_forward_cuda': [Case('forward_and_encode', _cdist_fwd, DET)],
    'cdist_encode': [Case('forward_and_encode', _cdist_fwd, DET)],
    'cdist_backward_cuda': [Case('centroids_without_gradient', _cdist_bwd, ATOMIC)],
    'pq_encode_heads': [Case('codes', _pq('codes'), DET)],
    'pq_loss_forward': [Case('loss_codes_gradients', _pq('single'), ATOMIC)],
    'pq_loss_backward': [Case('loss_codes_gradients', _pq('single'), ATOMIC)],
    'pq_loss_forward_pair': [Case('pair_loss_codes_gradients', _pq('pair'), ATOMIC)],
    'pq_loss_backward_pair': [Case('pair_loss_codes_gradients', _pq('pair'), ATOMIC)],
    'lookup_forward_cuda': [Case('z256_short_rows', _lookup, DET)],
    'sddmm_forward_cuda': [Case('ragged_duplicates', _sddmm, DET)],
    'spmm_forward_cuda': [Case('%s_%s' % ('t' if t else 'n', 'mfma' if m else 'gather'), _spmm(t, m), DET)
                          for t in (False, True) for m in (False, True)],
    'csr_transpose': [Case('ragged', _spmm_transposed(False), DET)],
    'transposed_for': [Case('ragged_memo', _spmm_transposed(True), DET)],
    'spmm_transposed': [Case('ragged', _spmm_transposed(False), DET)],
    'softmax_forward_cuda': [Case('ragged', _softmax('fwd'), DET)],
    'softmax_backward_cuda': [Case('ragged', _softmax('bwd'), DET)],
    'softmax_backward_clamped': [Case('ragged', _softmax('clamped'), DET)],
    'sparse_attention_forward': [Case('s%d_%s' % (s, 'yt' if yt else 'y'), _fused_attention(s, yt, True), DET)
                                 for s, yt in ((256, False), (160, True))],
    'sparse_attention_backward_rows': [Case('s160_yt', _fused_attention(160, True, True), DET)],
    'attention_mfma_prepare': [Case('s320_%s' % b, _mfma(1, 2, 320, 32, 64, False, b), ATOMIC)
                               for b in ('bits', 'counts')],
    'attention_mfma_forward': [Case('s640_e64_yt', _mfma(1, 2, 640, 64, 64, True), ATOMIC),
                               Case('s2048_z256_e64', _mfma(1, 1, 2048, 256, 64, False), ATOMIC)],
    'attention_mfma_backward': [Case('s320_e128', _mfma(1, 2, 320, 32, 128, False), ATOMIC),
                                Case('s320_e64_bf16_gt', _mfma(1, 2, 320, 32, 64, True, bf16=True), ATOMIC),
                                Case('s640_e64_16_heads', _mfma(1, 16, 640, 32, 64, False), ATOMIC)],
    'rotary': [Case('forward', _rotary(False), DET), Case('transposed', _rotary(True), DET)],
}

PARAMS = [pytest.param(entry, c, id='{}-{}'.format(entry, c.name)) for entry, cases in CASES.items() for c in cases]


def _flatten(outs):
    if isinstance(outs, torch.Tensor):
        return [outs]
    if outs is None:
        return []
    if hasattr(outs, 'buffer'):
        return [outs.buffer]
    flat = []
    for o in outs:
        flat += _flatten(o)
    return flat


def _run(call, pattern, memo):
    fresh_caches(*memo)
    with poisoned(pattern) as state:
        outs = call()
        torch.cuda.synchronize()
    assert not state.unclassified, 'uint8 workspaces of {} are not classified in tests/poison.py'.format(
        sorted(state.unclassified))
    return [o.clone() for o in _flatten(outs)], state


@pytest.mark.parametrize('entry,case', PARAMS)
def test_entry_ignores_what_its_buffers_held(entry, case):
    from naive_gpt import ext
    ext.load_library()
    built = case.build()
    call, check = built[0], built[1]
    memo = built[2] if len(built) > 2 else ()
    first, state = _run(call, 'zero', memo)
    assert state.count > 0, 'the poisoning reached no allocation'
    check(first)
    second, _ = _run(call, 'zero', memo)
    det = all(same_bits(a, b) for a, b in zip(first, second))
    assert det or case.kind == ATOMIC, '{}: classified {}, but two zero runs differ'.format(case.name, case.kind)
    for pattern in PATTERNS[1:]:
        outs, _ = _run(call, pattern, memo)
        if case.kind == DET:
            for i, (a, b) in enumerate(zip(first, outs)):
                assert same_bits(a, b), '{}: output {} under {} differs from the zero run'.format(
                    case.name, i, pattern)
        else:
            for i, o in enumerate(outs):
                assert not (o.is_floating_point() and torch.isnan(o).any()), \
                    '{}: NaN in output {} under {}'.format(case.name, i, pattern)
            check(outs)


# ---------------------------------------------------------------------------------------------------
# the step-level net: one forward and backward under every pattern

STEP_CONFIG = dict(d_model=256, n_heads=4, n_layers=1, max_length=256, vocab_size=512, d_feedforward=1024,
                   p_dropout=0.0)
STEP_BATCH = 8      # d_head 64 and n * h = 32 (the matrix-core attention), 2048 tokens (the fused head loss)


def _poisoned_runs(run):
    """run() -> (outputs, paths) under every pattern, from empty caches and path counts."""
    from naive_gpt import ext
    runs = {}
    for pattern in PATTERNS:
        fresh_caches()
        ext.reset_paths()
        with poisoned(pattern) as state:
            outs = run()
            torch.cuda.synchronize()
        assert state.count > 0 and not state.unclassified
        runs[pattern] = ([o.detach().clone() for o in outs], dict(ext.paths_taken()))
    base, paths = runs['zero']
    assert all(p == paths for _, p in runs.values()), 'the patterns took different paths'
    return runs


def _sites(paths, site):
    return {k[1] for k in paths if k[0] == site}


STEP_PATHS = (('attention', 'mfma'), ('routed_ffn', 'fused'), ('route_topk', 'kernel'), ('norm', 'kernel'),
              ('head_loss', 'fused'))


def model_step(kind):
    """(run, tuner) for the upgraded `kind` model of STEP_CONFIG on a STEP_BATCH batch: run() is one
    SparseTuner step -> [loss, every parameter gradient]; release the tuner when done."""
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    torch.manual_seed(0)
    model = utils.upgrade_sparse(checkpoint.build_model(kind, dict(STEP_CONFIG)), d_lora=16).cuda()
    gen = _gen(40)
    for name, p in model.named_parameters():
        if name.endswith('lora.right.weight'):          # a fresh adapter is the identity
            p.data.copy_(0.05 * torch.randn(p.shape, generator=gen).cuda())
    batch = torch.randint(0, STEP_CONFIG['vocab_size'], [STEP_BATCH, STEP_CONFIG['max_length'] + 2], generator=gen).cuda()
    tuner = utils.SparseTuner(model)
    model.train()

    def run():
        model.zero_grad(set_to_none=True)
        tuner.arm_triggers()
        loss = tuner.step_loss(batch[:, 1:-1], target=batch[:, 2:])      # as SparseTuner's eager step
        loss = loss + tuner.aux_weight * tuner.aux_loss()
        loss.backward()
        return [loss] + [p.grad for _, p in model.named_parameters() if p.grad is not None]
    return run, tuner


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_model_step_ignores_what_its_buffers_held(kind):
    """Loss and every parameter gradient of one SparseTuner step of an upgraded model on the default
    fused paths: matrix-core attention, fused routed FFN, fused norm, fused head loss, LoRA kernels.
    The attention backward sums grad_k / grad_v with float atomics (DET above does not hold for
    it), so outputs that differ in bits from the `zero` run are held to 1e-5 of scale instead; the
    layer-level tests below, which have no atomic path, require the same bits."""
    run, tuner = model_step(kind)
    try:
        runs = _poisoned_runs(run)
    finally:
        tuner.release()
    base, paths = runs['zero']
    for site, want in STEP_PATHS:
        assert _sites(paths, site) == {want}, (site, sorted(paths))
    assert len(base) > 10
    for pattern in PATTERNS[1:]:
        outs, _ = runs[pattern]
        for i, (a, b) in enumerate(zip(base, outs)):
            assert torch.isfinite(b).all(), '{}: output {} not finite under {}'.format(kind, i, pattern)
            if not same_bits(a, b):
                _close(b, a, 'step output {} under {}'.format(i, pattern), rtol=1e-5)


def _layer_runs(m, x, w):
    def run():
        for p in m.parameters():
            p.grad = None
        xi = x.detach().clone().requires_grad_(True)
        y = m(xi)
        (y * w).sum().backward()
        return [y, xi.grad] + [p.grad for p in m.parameters() if p.grad is not None]
    return _poisoned_runs(run)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_trainable_routed_layer_ignores_what_its_buffers_held(kind, bf16, monkeypatch):
    """grouped.TRAINABLE_WEIGHTS (as test_gpu_routed_train selects it) on the plain routed FFN, in
    fp32 and in bf16 storage: output, input gradient and every weight gradient in the same bits."""
    from naive_gpt.layers.sparse import grouped
    monkeypatch.setattr(grouped, 'TRAINABLE_WEIGHTS', True)
    if bf16:            # the shapes of test_gpu_routed_bf16 (bf16 storage: d and block multiples of 64)
        from test_gpu_routed_bf16 import _layer, _untied_tokens
        torch.manual_seed(5)
        m, k = _layer(kind, 192, 768, 192)
        x = _untied_tokens(m, k, 333, 192, 3)
        w = torch.randn(x.shape, generator=_gen(6)).cuda().to(torch.bfloat16)
    else:               # the reference golden layer of test_gpu_routed_train
        from test_gpu_routed_train import _golden_module
        m, z = _golden_module(kind)
        x = torch.from_numpy(z[kind + '.x'].astype(np.float32)).cuda()
        w = torch.from_numpy(z[kind + '.w'].astype(np.float32)).cuda()
    runs = _layer_runs(m, x, w)
    base, paths = runs['zero']
    assert _sites(paths, 'routed_ffn_plain') == {'grouped_trainable_bf16' if bf16 else 'grouped_trainable'}, paths
    assert _sites(paths, 'route_topk') == {'kernel'}, paths
    for pattern in PATTERNS[1:]:
        for i, (a, b) in enumerate(zip(base, runs[pattern][0])):
            assert same_bits(a, b), '{}: output {} under {} differs from the zero run'.format(kind, i, pattern)


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_lora_bf16_routed_layer_ignores_what_its_buffers_held(kind, monkeypatch):
    """grouped.LORA_BF16 (as test_gpu_routed_lora_bf16 selects it) on a bf16 LoRA routed FFN: the
    fused bf16 path, output, input gradient and every trained gradient in the same bits."""
    from naive_gpt.layers.sparse import grouped
    from test_gpu_routed_lora_bf16 import _clear_tokens, _lora_layer
    monkeypatch.setattr(grouped, 'LORA_BF16', True)
    d, dff, bs, r, T = 128, 512, 128, 16, 256
    m = _lora_layer(kind, d, dff, bs, r, seed=1)
    x = _clear_tokens(m, T, d, seed=2)
    w = torch.randn([T, d], generator=_gen(3)).cuda().to(torch.bfloat16)
    runs = _layer_runs(m, x, w)
    base, paths = runs['zero']
    assert _sites(paths, 'routed_ffn') == {'fused_bf16'}, paths
    for pattern in PATTERNS[1:]:
        for i, (a, b) in enumerate(zip(base, runs[pattern][0])):
            assert same_bits(a, b), '{}: output {} under {} differs from the zero run'.format(kind, i, pattern)
