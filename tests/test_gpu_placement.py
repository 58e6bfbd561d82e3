"""Every HIP entry of naive_gpt.ext at the weakest placement its contract accepts.

The other tiers give every operand the best possible place: an allocation of its own whose first
byte is 512-byte aligned, rows packed tight.  include/spt_hip.h promises less, and a real step gets
less: parameters are 16-byte slices of a tuner's flat buffer, q / k / v are column views of a joint
buffer, `out=` views and padded logits have a row stride above their width.  Here

* every case of test_gpu_guard_bands.PARAMS runs with every operand and every allocation 16 bytes
  past a 512-byte boundary (`guard.guarded(pattern, skew=16)`): 16 satisfies every alignment the
  header states and breaks every stronger one (32, 64, 128, 256, 512).  No operand of the header
  has a stated requirement above 16 bytes, so no entry gets another skew;
* SUB16: one case per operand whose stated alignment is below 16 bytes, at exactly that alignment:
  a view that starts that many bytes into a guarded allocation, against the same values at a
  16-byte aligned twin;
* PADDED: one pair per leading dimension / stride a caller can choose (test_placement_coverage holds
  the table against the header): tight rows, then rows padded by the smallest pad the header allows,
  NaN in the pad of inputs, a sentinel in the pad of outputs that must survive, and the value the C
  entry received recorded, so that a binding that copied to tight rows would be seen.

The oracle needs no tolerance: the same values at another address or behind a wider stride give the
same bits (DET), or pass the case's own check where float atomics leave the order open (ATOMIC).
The paths `ext.paths_taken()` reports must not change either: a path that changes with a placement
inside the contract is a silent fallback or an unstated requirement.  Every placement used here is one
the header documents as accepted, in memory the test owns between bands.

What this tier cannot see: a requirement that depends on the absolute address modulo more than 512.
"""
import contextlib
import ctypes
import sys

import pytest
import torch

import guard
import test_gpu_guard_bands as bands
import test_gpu_poisoned_buffers as suite
from poison import fresh_caches, same_bits
from test_gpu_guard_bands import _guarded_run, _guarded_steps, _verify
from test_gpu_poisoned_buffers import DET, _flatten, _gen

pytestmark = pytest.mark.gpu

SKEW = 16


def _paths_of(run):
    """run() from empty path counts -> (its result, the paths it took)"""
    from naive_gpt import ext
    ext.reset_paths()
    result = run()
    return result, dict(ext.paths_taken())


@pytest.mark.parametrize('entry,case', bands.PARAMS)
def test_entry_takes_operands_16_bytes_past_a_boundary(entry, case):
    from naive_gpt import ext
    ext.load_library()
    plain, plain_paths = _paths_of(lambda: bands._plain_run(case))
    for pattern in guard.PATTERNS:
        what = '{} ({}) at skew {} under {}'.format(entry, case.name, SKEW, pattern)
        try:
            (outs, check, state), paths = _paths_of(lambda: _guarded_run(case, pattern, what, skew=SKEW))
        except RuntimeError as err:
            raise AssertionError('{}: refused at a placement inside its contract: {}'.format(what, err)) from None
        print('placement {}-{} {}: allocations {} homes {} unguarded {}'.format(
            entry, case.name, pattern, state.allocations, state.homes, state.unguarded))
        assert state.allocations > 0, what + ': the guard reached no allocation'
        assert state.homes > 0, what + ': no operand went through _dev'
        assert state.unguarded == 0, what + ': allocations that could not be guarded'
        state.release()
        assert paths == plain_paths, '{}: took {} where the plain run took {}'.format(what, paths, plain_paths)
        assert len(outs) == len(plain), what
        if case.kind == DET:
            for i, (a, b) in enumerate(zip(plain, outs)):
                assert same_bits(a, b), '{}: output {} differs from the plain run'.format(what, i)
        else:
            for i, o in enumerate(outs):
                assert not (o.is_floating_point() and torch.isnan(o).any()), '{}: NaN in output {}'.format(what, i)
            check(outs)


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_model_step_takes_allocations_16_bytes_past_a_boundary(kind):
    """The twin of test_model_step_stays_inside_its_buffers: the same step, paths, bands and bounds, with
    every allocation of the guarded steps at skew 16."""
    _guarded_steps(kind, skew=SKEW)


# ---------------------------------------------------------------------------------------------------
# operands placed by hand: below 16 bytes, behind padded strides

SENTINEL = 12288.0                 # (exact in bf16 and fp16 too)
NAN = float('nan')


class Place:
    """The operands of one run, each in a guarded allocation of `state` (at its skew)."""

    def __init__(self, state):
        self.state, self.watched = state, []

    def dev(self, t):
        return guard.home(t, self.state, caller=sys._getframe(1).f_code.co_name)

    def at(self, t, nbytes):
        """t's values in a view that starts `nbytes` bytes into the allocation (NaN in front)"""
        k = nbytes // t.element_size()
        assert k * t.element_size() == nbytes and t.is_floating_point()
        flat = torch.full([t.numel() + k], NAN, dtype=t.dtype)
        flat[k:] = t.reshape(-1)
        v = self.dev(flat)[k:].view(t.shape)
        assert v.data_ptr() % 16 == (self.state.skew + nbytes) % 16
        return v

    def rows(self, t, pad):
        """a 2-D t behind a row stride of t.size(1) + pad elements, NaN in the pad"""
        parent = torch.full([t.size(0), t.size(1) + pad], NAN, dtype=t.dtype)
        parent[:, :t.size(1)] = t
        v = self.dev(parent)[:, :t.size(1)]
        assert v.stride(0) == t.size(1) + pad
        return v

    def spaced(self, ts, pad):
        """contiguous tensors of one shape one after the other, `pad` elements (NaN) between them"""
        n = ts[0].numel()
        flat = torch.full([len(ts) * (n + pad)], NAN, dtype=ts[0].dtype)
        for i, t in enumerate(ts):
            flat[i * (n + pad):i * (n + pad) + n] = t.reshape(-1)
        h = self.dev(flat)
        return [h[i * (n + pad):i * (n + pad) + n].view(ts[0].shape) for i in range(len(ts))]

    def out(self, shape, strides, dtype=torch.float32, extent=None):
        """an output view of these strides over an allocation full of SENTINEL; what lies between the
        live elements must still hold it after the call (check_outputs)"""
        extent = extent or 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        parent = self.dev(torch.full([extent], SENTINEL, dtype=dtype))
        view = parent.as_strided(shape, strides)
        self.watched.append((parent, view))
        return view

    def check_outputs(self, what):
        for parent, view in self.watched:
            live = torch.zeros_like(parent, dtype=torch.bool)
            live.as_strided(view.shape, view.stride()).fill_(True)
            assert (parent[~live] == SENTINEL).all(), what + ': a pad element of an output was written'


@contextlib.contextmanager
def recorded(entry):
    """The arguments the C entry receives, by parameter name, for as long as the block lasts: a wrapper
    set on the loaded library object."""
    from naive_gpt import ext
    from test_contract_refusals import prototypes
    lib, names, calls = ext.load_library(), prototypes()[entry], []
    real = getattr(lib, entry)

    def spy(*args):
        seen = dict(zip(names, args))
        for a in args:                  # a descriptor passed by reference: its fields, by name
            desc = getattr(a, '_obj', None)
            if isinstance(desc, ctypes.Structure):
                seen.update({name: getattr(desc, name) for name, _ in desc._fields_})
        calls.append(seen)
        return real(*args)
    setattr(lib, entry, spy)
    try:
        yield calls
    finally:
        setattr(lib, entry, real)


@contextlib.contextmanager
def allocating_at(nbytes, match):
    """Inside a guarded block: what torch.empty / empty_like create with match(shape, dtype) starts
    `nbytes` bytes into its guarded allocation -- an output the binding allocates itself, at the weakest
    alignment the header states for it.  The elements in front hold SENTINEL and are checked after."""
    empty, empty_like = torch.empty, torch.empty_like
    fronts = []

    def place(shape, dtype, device):
        k = nbytes // dtype.itemsize
        numel = 1
        for s in shape:
            numel *= s
        flat = empty([numel + k], dtype=dtype, device=device)
        flat[:k] = SENTINEL
        fronts.append(flat[:k])
        return flat[k:].view(list(shape))

    def at_empty(*size, **kw):
        shape = list(size[0]) if len(size) == 1 and not isinstance(size[0], int) else list(size)
        dtype = kw.get('dtype') or torch.float32
        if match(shape, dtype):
            return place(shape, dtype, kw.get('device'))
        return empty(*size, **kw)

    def at_empty_like(t, **kw):
        if not kw and t.is_contiguous() and match(list(t.shape), t.dtype):
            return place(t.shape, t.dtype, t.device)
        return empty_like(t, **kw)
    torch.empty, torch.empty_like = at_empty, at_empty_like
    try:
        yield fronts
    finally:
        torch.empty, torch.empty_like = empty, empty_like
    torch.cuda.synchronize()
    assert all((f == SENTINEL).all() for f in fronts), 'a store in front of an output at its stated alignment'


def _run_placed(build, variant, pattern, entries=()):
    """build(place, variant) -> call; the call inside guarded(pattern, skew=16)
    -> (outputs, {entry: the arguments of each of its calls}, paths)"""
    from naive_gpt import ext
    fresh_caches()
    ext.reset_paths()
    what = '{} {} under {}'.format(build.__name__, variant, pattern)
    with contextlib.ExitStack() as stack:
        state = stack.enter_context(guard.guarded(pattern, skew=SKEW))
        place = Place(state)
        try:
            call = build(place, variant)
            spies = {e: stack.enter_context(recorded(e)) for e in entries}
            outs = call()
        except RuntimeError as err:
            raise AssertionError('{}: refused at a placement inside its contract: {}'.format(what, err)) from None
        torch.cuda.synchronize()
    outs = [o.clone() for o in _flatten(outs)]
    _verify(state, what)
    place.check_outputs(what)
    print('placement {}: allocations {} homes {} unguarded {}'.format(what, state.allocations, state.homes,
                                                                      state.unguarded))
    assert state.homes > 0 and state.unguarded == 0, what
    state.release()
    for e, calls in spies.items():
        assert calls, '{}: {} was never called'.format(what, e)
    return outs, spies, dict(ext.paths_taken())


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x, y), '{}: output {} differs'.format(what, i)


def _randn(gen, *shape, dtype=torch.float32):
    return torch.randn(list(shape), generator=gen).to(dtype)


# ---- SUB16: operands whose stated alignment is below 16 bytes, at exactly that alignment.
# variant False: every operand 16-byte aligned (the twin); True: the named ones at their alignment.

def _sub16_rows_combine_bf16(p, low):
    """rows, bias (8 bytes) of spt_rows_combine_bf16, and its out (8 bytes; the binding allocates it)"""
    from naive_gpt import ext
    gen = _gen(50)
    T, k, d = 257, 2, 100
    put = (lambda t: p.at(t, 8)) if low else p.dev
    rows, bias = put(_randn(gen, T * k + 3, d, dtype=torch.bfloat16)), put(_randn(gen, d, dtype=torch.bfloat16))
    pos = p.dev(torch.randperm(T * k, generator=gen).int().view(T, k))

    def call():
        with allocating_at(8 if low else 0, lambda shape, dtype: shape == [T, d] and dtype == torch.bfloat16) as fronts:
            out = ext.rows_combine(rows, pos, bias=bias)
        assert len(fronts) == 1 and (not low or out.data_ptr() % 16 == 8)
        return out
    return call


def _sub16_gemm_bf16_epilogue(p, low):
    """bias, s_in and out (8 bytes) of spt_grouped_gemm_bf16's EPI_DACT epilogue"""
    from naive_gpt import ext
    gen = _gen(51)
    sizes, n, k = [0, 1, 0, 150, 0], 96, 64
    P, G = sum(sizes), len(sizes)
    put = (lambda t: p.at(t, 8)) if low else p.dev
    a, w = p.dev(_randn(gen, P, k, dtype=torch.bfloat16)), p.dev(_randn(gen, G * n, k, dtype=torch.bfloat16))
    bias, s_in = put(_randn(gen, G, n, dtype=torch.bfloat16)), put(_randn(gen, P, n, dtype=torch.bfloat16))
    off = p.dev(_offsets_cpu(sizes))

    def call():
        with allocating_at(8 if low else 0, lambda shape, dtype: shape == [P, n] and dtype == torch.bfloat16) as fronts:
            out = ext.grouped_gemm_bf16(a, w, off, G, n, k, n * k, k, 1, bias=bias, epilogue=ext.EPI_DACT,
                                        activation=ext.ACT_SILU, s_in=s_in)
        assert len(fronts) == 1
        return out
    return call


def _sub16_gemm_bf16_preact(p, low):
    """out and out2 (8 bytes) of spt_grouped_gemm_bf16's EPI_ACT epilogue"""
    from naive_gpt import ext
    gen = _gen(52)
    sizes, n, k = [0, 1, 0, 150, 0], 96, 64
    P, G = sum(sizes), len(sizes)
    a, w = p.dev(_randn(gen, P, k, dtype=torch.bfloat16)), p.dev(_randn(gen, G * n, k, dtype=torch.bfloat16))
    off = p.dev(_offsets_cpu(sizes))

    def call():
        with allocating_at(8 if low else 0, lambda shape, dtype: shape == [P, n] and dtype == torch.bfloat16) as fronts:
            out, preact = ext.grouped_gemm_bf16(a, w, off, G, n, k, n * k, k, 1, epilogue=ext.EPI_ACT,
                                                activation=ext.ACT_GELU, keep_preact=True)
        assert len(fronts) == 2
        return out, preact
    return call


def _sub16_gemm_bf16_ext_b2(p, low):
    """b2 (8 bytes) of spt_grouped_gemm_bf16_ext"""
    from naive_gpt import ext
    gen = _gen(53)
    sizes, n, k, r = [0, 1, 0, 150, 0], 96, 64, 16
    P, G = sum(sizes), len(sizes)
    a, w = p.dev(_randn(gen, P, k, dtype=torch.bfloat16)), p.dev(_randn(gen, G * n, k, dtype=torch.bfloat16))
    a2 = p.dev(_randn(gen, P, r))
    b2 = _randn(gen, G, n, r, dtype=torch.bfloat16)
    b2 = p.at(b2, 8) if low else p.dev(b2)
    off = p.dev(_offsets_cpu(sizes))
    return lambda: ext.grouped_gemm_bf16_ext(a, w, off, G, n, k, n * k, k, 1, a2, b2, n * r)


def _sub16_wgrad_bf16(p, low):
    """G, A, out (8 bytes) of spt_grouped_gemm_wgrad_bf16, and its dbias (the binding allocates it)"""
    from naive_gpt import ext
    gen = _gen(54)
    sizes, n, k = [0, 37, 0, 1, 300, 0], 100, 72
    P, G = sum(sizes), len(sizes)
    put = (lambda t: p.at(t, 8)) if low else p.dev
    grad, a = put(_randn(gen, P, n, dtype=torch.bfloat16)), put(_randn(gen, P, k, dtype=torch.bfloat16))
    scale = p.dev(torch.rand([P], generator=gen) + 0.5)
    off = p.dev(_offsets_cpu(sizes))
    out = put(torch.zeros([G * n * k], dtype=torch.bfloat16))

    def call():
        with allocating_at(8 if low else 0, lambda shape, dtype: shape == [G, n] and dtype == torch.bfloat16) as fronts:
            dw, dbias = ext.grouped_gemm_wgrad(grad, a, off, (n, k, n * k, k, 1), P, rowscale=scale, out=out,
                                               want_bias=True)
        assert len(fronts) == 1
        return dw, dbias
    return call


def _sub16_tall_tn_wide(p, low):
    """wide (8 bytes) of spt_tall_tn"""
    from naive_gpt import ext
    gen = _gen(55)
    sizes, width, n = [1, 63, 64, 65, 129, 0, 7], 64, 16
    rows = sum(sizes)
    wide = _randn(gen, rows, width)
    wide = p.at(wide, 8) if low else p.dev(wide)
    narrow, off = p.dev(_randn(gen, rows, n)), p.dev(_offsets_cpu(sizes))
    return lambda: ext.tall_tn(wide, narrow, offsets=off)


def _sub16_tall_tn_bf16(p, low):
    """wide (4 bytes) and out (2 bytes; the binding allocates it) of spt_tall_tn_bf16"""
    from naive_gpt import ext
    gen = _gen(56)
    sizes, width, n = [1, 63, 64, 65, 129, 0, 7], 64, 16
    rows, G = sum(sizes), len(sizes)
    wide = _randn(gen, rows, width, dtype=torch.bfloat16)
    wide = p.at(wide, 4) if low else p.dev(wide)
    narrow, off = p.dev(_randn(gen, rows, n)), p.dev(_offsets_cpu(sizes))

    def call():
        with allocating_at(2 if low else 0, lambda shape, dtype: shape == [G, width, n] and dtype == torch.bfloat16) as fronts:
            out = ext.tall_tn_bf16(wide, narrow, offsets=off)
        assert len(fronts) == 1 and (not low or out.data_ptr() % 4 == 2)
        return out
    return call


def _sub16_tall_tn_norm_params(p, low):
    """gammas / betas (8 bytes) of spt_tall_tn_norm"""
    from naive_gpt import ext
    gen = _gen(57)
    rows, width, n = 37, 768, 16
    s, narrow = p.dev(_randn(gen, rows, width)), p.dev(_randn(gen, rows, n))
    put = (lambda t: p.at(t, 8)) if low else p.dev
    gamma, beta = put(_randn(gen, width)), put(_randn(gen, width))
    mean, rstd = p.dev(_randn(gen, rows)), p.dev(torch.rand([rows], generator=gen) + 0.5)
    return lambda: ext.tall_tn(s, narrow, norm=(mean, rstd, gamma, beta))


def _sub16_swiglu_bf16(p, low):
    """the bf16 tensors (8 bytes) and the dots (4 bytes; the binding allocates them) of
    spt_swiglu_backward_dots_bf16, and of the elementwise pair"""
    from naive_gpt import ext
    gen = _gen(58)
    rows, n = 33, 100
    put = (lambda t: p.at(t, 8)) if low else p.dev
    g, s, dh = (put(_randn(gen, rows, n, dtype=torch.bfloat16)) for _ in range(3))

    def call():
        with allocating_at(4 if low else 0, lambda shape, dtype: shape == [3, rows]) as fronts:
            dots = ext.swiglu_backward_dots_bf16(dh, g, s)
        assert len(fronts) == 1
        with allocating_at(8 if low else 0, lambda shape, dtype: shape == [rows, n] and dtype == torch.bfloat16) as fronts:
            plain = ext.swiglu_forward_bf16(g, s), ext.swiglu_backward_bf16(dh, g, s)
        assert len(fronts) == 3
        return dots, plain
    return call


def _sub16_lora_down_bf16_tables(p, low):
    """l (8 bytes) of spt_lora_down_bf16 and spt_lora_down_grouped_bf16"""
    from naive_gpt import ext
    gen = _gen(59)
    sizes, K, n = [0, 300, 0, 1, 200, 0], 64, 20
    rows, G = sum(sizes), len(sizes)
    put = (lambda t: p.at(t, 8)) if low else p.dev
    x = p.dev(_randn(gen, rows, K, dtype=torch.bfloat16))
    table, tables = put(_randn(gen, K, n, dtype=torch.bfloat16)), put(_randn(gen, G, K, n, dtype=torch.bfloat16))
    off = p.dev(_offsets_cpu(sizes))
    return lambda: (ext.lora_down_bf16(x, table), ext.lora_down_grouped_bf16(x, tables, off))


def _sub16_gemm_w16(p, low):
    """w (fp16, 8 bytes) of spt_grouped_gemm_fused_w16"""
    from naive_gpt import ext
    gen = _gen(60)
    rows, k, G, n = 33, 64, 1, 96
    x = p.dev(_randn(gen, rows, k))
    w = _randn(gen, G * n, k, dtype=torch.float16)
    w16 = p.at(w, 8) if low else p.dev(w)
    image = ext.split_bf16(p.dev(w))          # (the image of an aligned copy: spt_split_f16 wants 16 bytes)
    off = p.dev(_offsets_cpu([rows]))
    a_norm, w_norm = p.dev(x.norm(dim=1).cpu()), p.dev(w.float().norm(dim=1))      # (the ReLU epilogue reads w itself)
    return lambda: ext.grouped_gemm_fused(x, w16, off, G, n=n, k=k, w_group_stride=n * k, w_ldn=k, w_ldk=1, n_rows=rows,
                                          w_image=image, epilogue=ext.EPI_ACT, activation=ext.ACT_RELU,
                                          a_norm=a_norm, w_norm=w_norm)


def _offsets_cpu(sizes):
    import numpy as np
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)


SUB16 = [_sub16_rows_combine_bf16, _sub16_gemm_bf16_epilogue, _sub16_gemm_bf16_preact, _sub16_gemm_bf16_ext_b2,
         _sub16_wgrad_bf16, _sub16_tall_tn_wide, _sub16_tall_tn_bf16, _sub16_tall_tn_norm_params, _sub16_swiglu_bf16,
         _sub16_lora_down_bf16_tables, _sub16_gemm_w16]


@pytest.mark.parametrize('build', SUB16, ids=lambda b: b.__name__[7:])
def test_operand_at_its_stated_alignment_below_16_bytes(build):
    for pattern in guard.PATTERNS:
        twin, _, twin_paths = _run_placed(build, False, pattern)
        outs, _, paths = _run_placed(build, True, pattern)
        assert paths == twin_paths, (build.__name__, paths, twin_paths)
        _same(twin, outs, '{} under {}: at the stated alignment against the 16-byte aligned twin'.format(
            build.__name__, pattern))


# ---- PADDED: a leading dimension or stride a caller chooses, tight and then padded by the smallest pad
# the header allows.  build(place, padded) -> call; the table maps (C entry, parameter) -> case.

def _pad_grouped_gemm(p, padded):
    """lda % 4 == 0; w_group_stride % 4 == 0: the groups' weights 4 floats apart"""
    from naive_gpt import ext
    gen = _gen(70)
    sizes, n, k, T = suite.GG_SIZES, 200, 72, 190
    P, G = sum(sizes), len(sizes)
    pad = 4 if padded else 0
    a = p.rows(_randn(gen, T, k), pad)
    w = p.spaced(list(_randn(gen, G, n * k).unbind(0)), pad)[0]
    weight = w.as_strided([G * (n * k + pad) - pad], [1])
    bias, scale = p.dev(_randn(gen, G, n)), p.dev(torch.rand([P], generator=gen) + 0.5)
    gather = p.dev(torch.randint(0, T, [P], generator=gen, dtype=torch.int32))
    off = p.dev(_offsets_cpu(sizes))
    return lambda: ext.grouped_gemm(a, weight, off, G, n, k, n * k + pad, k, 1, gather=gather, bias=bias,
                                    rowscale=scale)


def _pad_wgrad(dtype):
    def _pad_wgrad_of(p, padded):
        """ldg, lda, ldn, group_stride % 4 == 0 (fp32 and bf16 alike): each 4 elements above its tight value;
        out in the padded layout of the view, SENTINEL between its live elements"""
        from naive_gpt import ext
        gen = _gen(71)
        sizes, n, k = [0, 37, 0, 1, 300, 0], 100, 72
        P, G = sum(sizes), len(sizes)
        pad = 4 if padded else 0
        grad, a = p.rows(_randn(gen, P, n, dtype=dtype), pad), p.rows(_randn(gen, P, k, dtype=dtype), pad)
        scale = p.dev(torch.rand([P], generator=gen) + 0.5)
        off = p.dev(_offsets_cpu(sizes))
        ldn = k + pad
        gstride = n * ldn + pad
        live = p.out([G, n, k], [gstride, ldn, 1], dtype=dtype)
        out = live.as_strided([(G - 1) * gstride + (n - 1) * ldn + k], [1])

        def call():
            _, dbias = ext.grouped_gemm_wgrad(grad, a, off, (n, k, gstride, ldn, 1), P, rowscale=scale, out=out,
                                              want_bias=True)
            return live, dbias
        return call
    _pad_wgrad_of.__name__ = '_pad_wgrad_' + str(dtype).split('.')[-1]
    return _pad_wgrad_of


_pad_wgrad_fp32, _pad_wgrad_bf16 = _pad_wgrad(torch.float32), _pad_wgrad(torch.bfloat16)


def _pad_split(dtype, step):
    def _pad_split_of(p, padded):
        """ld % 4 == 0 (fp32), ld % 8 == 0 (halves)"""
        from naive_gpt import ext
        x = p.rows(_randn(_gen(72), 33, 40, dtype=dtype), step if padded else 0)
        return lambda: ext.split_bf16(x).buffer
    _pad_split_of.__name__ = '_pad_split_' + str(dtype).split('.')[-1]
    return _pad_split_of


_pad_split_fp32, _pad_split_f16 = _pad_split(torch.float32, 4), _pad_split(torch.float16, 8)


def _pad_lora_down(p, padded):
    """ldx % 4 == 0; ldu: any row stride >= n (a column slice of a wider matrix): n + 1"""
    from naive_gpt import ext
    gen = _gen(73)
    rows, K, n = 1000, 96, 32
    x, t = p.rows(_randn(gen, rows, K), 4 if padded else 0), p.dev(_randn(gen, K, n))
    u = p.out([rows, n], [n + (1 if padded else 0), 1])

    def call():
        ext.lora_down(x, t, out=u)
        return u, ext.lora_down(x, t, want_image=True, want_norms=True, exact=True)
    return call


def _pad_lora_down2(route):
    def _pad_lora_down2_of(p, padded):
        """ldx % 4 == 0"""
        from naive_gpt import ext
        gen = _gen(74)
        rows, K, n, n2 = 1000, 96, 16, 5
        x, t = p.rows(_randn(gen, rows, K), 4 if padded else 0), p.dev(_randn(gen, K, n))
        t2, bias = p.dev(_randn(gen, n2, K) / 16), p.dev(_randn(gen, n2))
        return lambda: ext.lora_down(x, t, block_major=True, exact=True, table2=t2, want_image=True,
                                     route=(bias, 2) if route else None)
    _pad_lora_down2_of.__name__ = '_pad_lora_down2' + ('_route' if route else '')
    return _pad_lora_down2_of


_pad_lora_down2_plain, _pad_lora_down2_route = _pad_lora_down2(False), _pad_lora_down2(True)


def _pad_lora_down_tables(p, padded):
    """ldx % 4 == 0; table_stride % 4 == 0: the tables 4 floats further apart"""
    from naive_gpt import ext
    gen = _gen(75)
    rows, K = 777, 64
    x = p.rows(_randn(gen, rows, K), 4 if padded else 0)
    tables = p.spaced(list(_randn(gen, 3, K, 16).unbind(0)), 4 if padded else 0)

    def call():
        u, img = ext.lora_down_tables(x, tables, want_image=True)
        return u, img.buffer
    return call


def _pad_lora_down_stacked(p, padded):
    """l_group_stride (the tables' spacing) and ldu % 4 == 0; the stacked inputs stay back to back"""
    from naive_gpt import ext
    gen = _gen(76)
    G, rows, K = 3, 333, 64
    xs = list(p.dev(_randn(gen, G, rows, K)).unbind(0))
    tables = p.spaced(list(_randn(gen, G, K, 16).unbind(0)), 4 if padded else 0)
    off = p.dev(torch.arange(0, G * rows + 1, rows, dtype=torch.int32))
    out = p.out([rows, 16 * G], [16 * G + (4 if padded else 0), 1])
    return lambda: ext.lora_down_stacked(xs, tables, off, out)


def _pad_lora_down_stacked_one(p, padded):
    """ldx % 4 == 0 of spt_lora_down_grouped_cols: one group, whose input need not be packed"""
    from naive_gpt import ext
    gen = _gen(77)
    rows, K = 333, 64
    x, t = p.rows(_randn(gen, rows, K), 4 if padded else 0), p.dev(_randn(gen, K, 16))
    off = p.dev(torch.tensor([0, rows], dtype=torch.int32))
    out = p.out([rows, 16], [16, 1])
    return lambda: ext.lora_down_stacked([x], [t], off, out)


def _pad_lora_down_grouped(p, padded):
    """ldx % 4 == 0"""
    from naive_gpt import ext
    gen = _gen(78)
    sizes, K, n = [0, 300, 0, 1, 200, 0], 64, 16
    x = p.rows(_randn(gen, sum(sizes), K), 4 if padded else 0)
    tables, off = p.dev(_randn(gen, len(sizes), K, n)), p.dev(_offsets_cpu(sizes))

    def call():
        u, img = ext.lora_down_grouped(x, tables, off, want_image=True)
        return u, img.buffer
    return call


def _pad_lora_down_bf16(p, padded):
    """ldx % 8 == 0 of spt_lora_down_bf16 and spt_lora_down_grouped_bf16"""
    from naive_gpt import ext
    gen = _gen(79)
    sizes, K, n = [0, 300, 0, 1, 200, 0], 64, 16
    x = p.rows(_randn(gen, sum(sizes), K, dtype=torch.bfloat16), 8 if padded else 0)
    table = p.dev(_randn(gen, K, n, dtype=torch.bfloat16))
    tables, off = p.dev(_randn(gen, len(sizes), K, n, dtype=torch.bfloat16)), p.dev(_offsets_cpu(sizes))
    return lambda: (ext.lora_down_bf16(x, table), ext.lora_down_bf16(x, table, block_major=True),
                    ext.lora_down_grouped_bf16(x, tables, off))


def _pad_cross_entropy(p, padded):
    """ld % 4 == 0.  The head loss works in place and the header gives it the pad columns: it writes zeros
    there (asserted), so they start as NaN, not as a sentinel"""
    from naive_gpt import ext
    gen = _gen(80)
    rows, V = 33, 1000
    z = 3.0 * torch.randn([rows, V], generator=gen)
    target = torch.randint(0, V, [rows], generator=gen)
    target[::4] = -100
    scale = p.dev((1.0 / (target != -100).sum().float()).reshape(1))
    target = p.dev(target)
    held, grads = p.rows(z, 4 if padded else 0), p.rows(z, 4 if padded else 0)

    def call():
        loss, top = ext.cross_entropy_grad_(held, V, target, None, evaluate=True)
        kept = held.clone()
        loss2 = ext.cross_entropy_grad_(grads, V, target, scale)
        if padded:
            parent = grads.as_strided([rows, V + 4], [V + 4, 1])
            assert (parent[:, V:] == 0).all(), 'pad columns of the gradient are not 0'
        return loss, top, kept, loss2, grads
    return call


def _pad_tall_tn(which):
    def _pad_tall_tn_of(p, padded):
        """ldw even: + 2; ldn % 4 == 0: + 4 (norm: ldn2 % 4 == 0 too)"""
        from naive_gpt import ext
        gen = _gen(81)
        sizes, width, n = [1, 63, 64, 65, 129, 0, 7], 64, 16
        if which == 'norm':
            sizes, width = [37], 768
        rows = sum(sizes)
        dt = torch.bfloat16 if which == 'bf16' else torch.float32
        wides = [p.rows(_randn(gen, rows, width, dtype=dt), 2 if padded else 0) for _ in range(2)]
        narrows = [p.rows(_randn(gen, rows, n), 4 if padded else 0) for _ in range(2)]
        off = p.dev(_offsets_cpu(sizes))
        if which == 'single':
            return lambda: ext.tall_tn(wides[0], narrows[0], offsets=off)
        if which == 'batch':
            return lambda: ext.tall_tn_batch(wides, narrows, offsets=off)
        if which == 'bf16':
            return lambda: ext.tall_tn_bf16(wides[0], narrows[0], offsets=off)
        narrows2 = [p.rows(_randn(gen, rows, 4), 4 if padded else 0) for _ in range(2)]
        norm = (p.dev(_randn(gen, rows)), p.dev(torch.rand([rows], generator=gen) + 0.5), p.dev(_randn(gen, width)),
                p.dev(_randn(gen, width)))
        return lambda: ext.tall_tn_batch(wides, narrows, norms=[norm, None], narrows2=narrows2)
    _pad_tall_tn_of.__name__ = '_pad_tall_tn_' + which
    return _pad_tall_tn_of


_pad_tall_tn_single, _pad_tall_tn_batch, _pad_tall_tn_bf16, _pad_tall_tn_norm = (
    _pad_tall_tn(w) for w in ('single', 'batch', 'bf16', 'norm'))


def _pad_route_logits(p, padded):
    """ld >= n_blocks (the binding: a multiple of 4): 8 and 12 for 8 blocks -- the logits and the counts of
    one spt_lora_down2_route launch, whose own logits have ld 16"""
    from naive_gpt import ext
    gen = _gen(82)
    rows, K, G, k = 300, 64, 8, 2
    x, t, router = p.dev(_randn(gen, rows, K)), p.dev(_randn(gen, K, 16)), p.dev(_randn(gen, G, K) / 8)
    bias = p.dev(torch.rand([G], generator=gen) * 0.01)
    u, _, _, counts = ext.lora_down(x, t, block_major=True, exact=True, table2=router, route=(bias, k))
    torch.cuda.synchronize()
    logits = p.rows(u[-1][:, :G].cpu(), 4 if padded else 0)
    return lambda: (ext.route_topk_logits(logits, bias, G, k, 2.0),
                    ext.route_topk_logits(logits, bias, G, k, 2.0, counts=counts))


def _pad_embedding_rows(p, padded):
    """ldg % 4 == 0"""
    from naive_gpt import ext
    gen = _gen(83)
    rows, T, width = 50, 40, 24
    ids = p.dev(torch.tensor([3, 7, 11, 49])[torch.randint(0, 4, [T], generator=gen)])
    g = p.rows(_randn(gen, T, width), 4 if padded else 0)
    return lambda: ext.embedding_rows_backward(g, ids, rows)


def _pad_gemm_fused(w16):
    def _pad_gemm_fused_of(p, padded):
        """SptGroupedGemm: lda, lda2, b2_group_stride % 4 == 0: + 4; w_group_stride % 4 == 0: + 4 (halves: the
        image path wants whole weight rows and % 32: + one row of k = 96); ldo >= n: n + 1"""
        from naive_gpt import ext
        gen = _gen(84)
        sizes, n, k, r = [0, 1, 0, 150, 0], 200, 96, 16
        P, G = sum(sizes), len(sizes)
        pad = 4 if padded else 0
        wpad = (k if w16 else 4) if padded else 0
        a, a2 = p.rows(_randn(gen, P, k), pad), p.rows(_randn(gen, P, r), pad)
        w = _randn(gen, G, n * k, dtype=torch.float16 if w16 else torch.float32)
        first = p.spaced(list(w.unbind(0)), wpad)[0]
        weight = first.as_strided([G * (n * k + wpad) - wpad], [1])
        b2 = p.spaced(list(_randn(gen, G, n, r).unbind(0)), pad)[0]
        bias, scale = p.dev(_randn(gen, G, n)), p.dev(torch.rand([P], generator=gen) + 0.5)
        off = p.dev(_offsets_cpu(sizes))
        image = None
        if w16:                      # the image of the whole weight as it lies in memory, pad rows and all
            weight = weight.view(-1, k)
            weight[torch.isnan(weight)] = 0            # (the image is made from every row; the GEMM reads the groups')
            image = ext.split_bf16(weight)
        out = p.out([P, n], [n + (1 if padded else 0), 1])
        return lambda: ext.grouped_gemm_fused(a, weight, off, G, n=n, k=k, w_group_stride=n * k + wpad, w_ldn=k, w_ldk=1,
                                              n_rows=P, bias=bias, rowscale=scale, a2=a2, b2=b2,
                                              b2_group_stride=n * r + pad, w_image=image, out=out)
    _pad_gemm_fused_of.__name__ = '_pad_gemm_fused' + ('_w16' if w16 else '')
    return _pad_gemm_fused_of


def _pad_gemm_segments(w16):
    def _pad_gemm_segments_of(p, padded):
        """SptGroupedGemm: a_seg_stride % 4 == 0 and b2_seg_stride % 4 == 0: the three segments of `a`, and the
        three rank-16 tables, 4 floats further apart"""
        from naive_gpt import ext
        gen = _gen(85)
        sizes, n, seg_k, r = [100, 50], 96, 32, 48
        P, G, k = sum(sizes), len(sizes), 3 * seg_k
        pad = 4 if padded else 0
        segs = p.spaced(list(_randn(gen, 3, P, seg_k).unbind(0)), pad)
        tables = p.spaced(list(_randn(gen, 3, n, 16).unbind(0)), pad)
        a2 = p.dev(_randn(gen, P, r))
        w = _randn(gen, G * n, k, dtype=torch.float16 if w16 else torch.float32)
        weight = p.dev(w)
        image = ext.split_bf16(weight) if w16 else None
        off = p.dev(_offsets_cpu(sizes))
        return lambda: ext.grouped_gemm_fused(segs[0], weight, off, G, n=n, k=k, w_group_stride=n * k, w_ldn=k, w_ldk=1,
                                              n_rows=P, a2=a2, b2=tables[0], w_image=image,
                                              a_segments=(seg_k, P * seg_k + pad), b2_segment_stride=n * 16 + pad)
    _pad_gemm_segments_of.__name__ = '_pad_gemm_segments' + ('_w16' if w16 else '')
    return _pad_gemm_segments_of


def _pad_gemm_bf16(p, padded):
    """SptGroupedGemmBf16 (+ Ext): lda, w_group_stride % 8 == 0: + 8; lda2, b2_group_stride % 4 == 0: + 4; ldo:
    + 4, which keeps the rows of out at the 8 bytes stated for it"""
    from naive_gpt import ext
    gen = _gen(86)
    sizes, n, k, r = [0, 1, 0, 150, 0], 96, 64, 16
    P, G = sum(sizes), len(sizes)
    a = p.rows(_randn(gen, P, k, dtype=torch.bfloat16), 8 if padded else 0)
    a2 = p.rows(_randn(gen, P, r), 4 if padded else 0)
    first = p.spaced(list(_randn(gen, G, n * k, dtype=torch.bfloat16).unbind(0)), 8 if padded else 0)[0]
    weight = first.as_strided([G * (n * k + 8) - 8 if padded else G * n * k], [1])
    b2 = p.spaced(list(_randn(gen, G, n * r, dtype=torch.bfloat16).unbind(0)), 4 if padded else 0)[0]
    b2 = b2.as_strided([G * (n * r + 4) - 4 if padded else G * n * r], [1])
    off = p.dev(_offsets_cpu(sizes))
    gs, b2s = n * k + (8 if padded else 0), n * r + (4 if padded else 0)
    out, out2 = (p.out([P, n], [n + (4 if padded else 0), 1], dtype=torch.bfloat16) for _ in range(2))
    return lambda: (ext.grouped_gemm_bf16(a, weight, off, G, n, k, gs, k, 1, out=out),
                    ext.grouped_gemm_bf16_ext(a, weight, off, G, n, k, gs, k, 1, a2, b2, b2s, out=out2))


_pad_gemm_fused_fp32, _pad_gemm_fused_w16 = _pad_gemm_fused(False), _pad_gemm_fused(True)
_pad_gemm_segments_fp32, _pad_gemm_segments_w16 = _pad_gemm_segments(False), _pad_gemm_segments(True)

PADDED = {
    ('spt_grouped_gemm', 'lda'): _pad_grouped_gemm, ('spt_grouped_gemm', 'w_group_stride'): _pad_grouped_gemm,
    ('spt_split_bf16', 'ld'): _pad_split_fp32, ('spt_split_f16', 'ld'): _pad_split_f16,
    ('spt_lora_down', 'ldx'): _pad_lora_down, ('spt_lora_down', 'ldu'): _pad_lora_down,
    ('spt_lora_down2', 'ldx'): _pad_lora_down2_plain, ('spt_lora_down2_route', 'ldx'): _pad_lora_down2_route,
    ('spt_lora_down_tables', 'ldx'): _pad_lora_down_tables,
    ('spt_lora_down_tables', 'table_stride'): _pad_lora_down_tables,
    ('spt_lora_down_grouped_cols', 'ldx'): _pad_lora_down_stacked_one,
    ('spt_lora_down_grouped_cols', 'l_group_stride'): _pad_lora_down_stacked,
    ('spt_lora_down_grouped_cols', 'ldu'): _pad_lora_down_stacked,
    ('spt_lora_down_grouped', 'ldx'): _pad_lora_down_grouped,
    ('spt_lora_down_bf16', 'ldx'): _pad_lora_down_bf16, ('spt_lora_down_grouped_bf16', 'ldx'): _pad_lora_down_bf16,
    ('spt_cross_entropy_grad', 'ld'): _pad_cross_entropy, ('spt_cross_entropy_eval', 'ld'): _pad_cross_entropy,
    ('spt_tall_tn', 'ldw'): _pad_tall_tn_single, ('spt_tall_tn', 'ldn'): _pad_tall_tn_single,
    ('spt_tall_tn_batch', 'ldw'): _pad_tall_tn_batch, ('spt_tall_tn_batch', 'ldn'): _pad_tall_tn_batch,
    ('spt_tall_tn_norm', 'ldw'): _pad_tall_tn_norm, ('spt_tall_tn_norm', 'ldn'): _pad_tall_tn_norm,
    ('spt_tall_tn_norm', 'ldn2'): _pad_tall_tn_norm,
    ('spt_tall_tn_bf16', 'ldw'): _pad_tall_tn_bf16, ('spt_tall_tn_bf16', 'ldn'): _pad_tall_tn_bf16,
    ('spt_route_topk_logits', 'ld'): _pad_route_logits, ('spt_route_topk_counted', 'ld'): _pad_route_logits,
    ('spt_embedding_rows_backward', 'ldg'): _pad_embedding_rows,
}
# ... and the descriptors' fields, under the entry that takes the descriptor
for _entry, _plain, _segments in (('spt_grouped_gemm_fused', _pad_gemm_fused_fp32, _pad_gemm_segments_fp32),
                                  ('spt_grouped_gemm_fused_w16', _pad_gemm_fused_w16, _pad_gemm_segments_w16)):
    for _param in ('lda', 'w_group_stride', 'lda2', 'b2_group_stride', 'ldo'):
        PADDED[(_entry, _param)] = _plain
    for _param in ('a_seg_stride', 'b2_seg_stride'):
        PADDED[(_entry, _param)] = _segments
for _param in ('lda', 'w_group_stride', 'ldo'):
    PADDED[('spt_grouped_gemm_bf16', _param)] = PADDED[('spt_grouped_gemm_bf16_ext', _param)] = _pad_gemm_bf16
for _param in ('lda2', 'b2_group_stride'):
    PADDED[('spt_grouped_gemm_bf16_ext', _param)] = _pad_gemm_bf16
for _entry in ('spt_grouped_gemm_wgrad', 'spt_grouped_gemm_wgrad_bf16'):
    for _param in ('ldg', 'lda', 'group_stride', 'ldn'):
        PADDED[(_entry, _param)] = _pad_wgrad_bf16 if _entry.endswith('bf16') else _pad_wgrad_fp32

# A caller of naive_gpt.ext cannot give these another value than the tight one
TIGHT_ONLY = {
    ('spt_lora_down2', 'ldu'): 'the binding passes 0 (= n): it allocates the block-major u itself and takes no out=',
    ('spt_lora_down2_route', 'ldu'): 'the binding passes 0 (= n): it allocates the block-major u itself',
    ('spt_lora_down_grouped', 'l_group_stride'): 'k * n of a tables tensor the binding requires contiguous',
    ('spt_lora_down_grouped', 'ldu'): 'the binding passes 0 (= n): it allocates u itself and takes no out=',
    ('spt_lora_down_bf16', 'ldu'): 'the binding passes 0 (= n): it allocates u itself and takes no out=',
    ('spt_lora_down_grouped_bf16', 'l_group_stride'): 'k * n of a tables tensor the binding requires contiguous',
    ('spt_lora_down_grouped_bf16', 'ldu'): 'the binding passes 0 (= n): it allocates u itself and takes no out=',
    ('spt_rotary', 'out_stride'): 'numel() of one part: the binding allocates the parts\' buffer itself, packed',
    ('spt_embedding_rows_backward', 'ldo'): 'the width of the out the binding allocates itself, packed',
}


def _cases():
    cases = {}
    for key, build in PADDED.items():
        cases.setdefault(build, []).append(key)
    return [pytest.param(build, keys, id=build.__name__[5:]) for build, keys in cases.items()]


@pytest.mark.parametrize('build,keys', _cases())
def test_padded_leading_dimension_gives_the_bits_of_tight_rows(build, keys):
    entries = sorted({e for e, _ in keys})
    for pattern in guard.PATTERNS:
        tight, seen_tight, tight_paths = _run_placed(build, False, pattern, entries)
        outs, seen, paths = _run_placed(build, True, pattern, entries)
        for entry, param in keys:
            got, tight_got = [c[param] for c in seen[entry]], [c[param] for c in seen_tight[entry]]
            assert len(got) == len(tight_got) and any(a > b for a, b in zip(got, tight_got)), \
                '{}: {} received {} = {} in the padded run, {} in the tight one: the binding did not pass the ' \
                'padded rows on'.format(build.__name__, entry, param, got, tight_got)
        assert paths == tight_paths, (build.__name__, paths, tight_paths)
        _same(tight, outs, '{} under {}: padded against tight rows'.format(build.__name__, pattern))
