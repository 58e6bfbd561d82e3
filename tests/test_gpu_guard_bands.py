"""Every HIP entry of naive_gpt.ext between guard bands: no access outside its buffers
(tests/guard.py).

Each case of test_gpu_poisoned_buffers.CASES, the d_head-80 attention cases and the fused add + norm
kernels' other forms run once plainly and once under each band pattern.  In the guarded runs every
operand lies in a guarded allocation of its own (`_dev` of the registry swapped for guard.home), and
so does every output, scratch and workspace the wrapper allocates.  Then

* a band that changed is a store outside a buffer;
* DET cases: bits that differ from the plain run, in any output and under either pattern, are a
  result that depends on bytes outside an input;
* ATOMIC cases (float atomics in no fixed order): a NaN is the same thing, and the outputs pass the
  case's reference check again.

The bands are memory the test owns, and integer bands hold 0 or 1: an access this tier can catch
faults nothing, and an over-read index stays a valid one.
"""
import sys

import pytest
import torch

import guard
import test_gpu_mfma_attention_e80 as e80
import test_gpu_poisoned_buffers as suite
from poison import fresh_caches, same_bits
from test_gpu_poisoned_buffers import ATOMIC, DET, Case, _close, _flatten, _layernorm, _sites

pytestmark = pytest.mark.gpu

# the one-wave-per-row form (768) and the wide-row forms (2560: two waves, 5120: four) at one row and
# at 37: the smallest counts that leave a workgroup's round of rows ragged
LAYERNORM_CASES = [('add_layernorm_forward', Case('d%d_rows_%d_%s' % (d, r, 'rms' if m else 'ln'), _layernorm(r, m, d), DET))
                   for d in (768, 2560, 5120) for r in (37, 1) for m in (False, True)]

PARAMS = suite.PARAMS + [pytest.param(entry, c, id='{}-{}'.format(entry, c.name))
                         for entry, c in e80.E80_CASES + LAYERNORM_CASES]


def _verify(state, what):
    try:
        state.verify()
    except AssertionError as err:
        raise AssertionError('{}: {}'.format(what, err)) from None


def _plain_run(case):
    built = case.build()
    call, check = built[0], built[1]
    fresh_caches(*(built[2] if len(built) > 2 else ()))
    outs = call()
    torch.cuda.synchronize()
    outs = [o.clone() for o in _flatten(outs)]
    check(outs)
    return outs


def _guarded_run(case, pattern, what, skew=0):
    """build() and call() with every operand and every allocation between bands of `pattern`, its
    first byte `skew` bytes past a 512-byte boundary (test_gpu_placement: 16)
    -> (outputs, the build's check, the guard's state), the bands verified."""
    fresh_caches()
    with guard.guarded(pattern, skew=skew) as state:
        def to_home(t):
            return guard.home(t, state, caller=sys._getframe(1).f_code.co_name)
        plain_dev, suite._dev = suite._dev, to_home
        try:
            built = case.build()
            memo = built[2] if len(built) > 2 else ()
            fresh_caches(*memo)
            outs = built[0]()
            torch.cuda.synchronize()
        finally:
            suite._dev = plain_dev
    outs = [o.clone() for o in _flatten(outs)]
    _verify(state, what)
    fresh_caches(*memo)
    return outs, built[1], state


@pytest.mark.parametrize('entry,case', PARAMS)
def test_entry_stays_inside_its_buffers(entry, case):
    from naive_gpt import ext
    ext.load_library()
    plain = _plain_run(case)
    for pattern in guard.PATTERNS:
        what = '{} ({}) under {}'.format(entry, case.name, pattern)
        outs, check, state = _guarded_run(case, pattern, what)
        print('guard {}-{} {}: allocations {} homes {} unguarded {}'.format(
            entry, case.name, pattern, state.allocations, state.homes, state.unguarded))
        assert state.allocations > 0, what + ': the guard reached no allocation'
        assert state.homes > 0, what + ': no operand went through _dev'
        assert state.unguarded == 0, what + ': allocations that could not be guarded'
        state.release()
        assert len(outs) == len(plain), what
        if case.kind == DET:
            for i, (a, b) in enumerate(zip(plain, outs)):
                assert same_bits(a, b), \
                    '{}: output {} differs from the plain run: it depends on bytes outside an input'.format(what, i)
        else:
            for i, o in enumerate(outs):
                assert not (o.is_floating_point() and torch.isnan(o).any()), \
                    '{}: NaN in output {}: it depends on bytes outside an input'.format(what, i)
            check(outs)


def _guarded_steps(kind, skew=0):
    """One SparseTuner step of the upgraded model of test_model_step_ignores_what_its_buffers_held,
    on the same paths, with every allocation of the step between 64 KiB bands (the state keeps them
    all alive until verify(); parameters and the batch stay where they are).  Loss and gradients
    within that test's 1e-5 of the unguarded step, not in the same bits: the attention backward's
    atomics are the same exception as there.  `skew`: of every allocation of the guarded steps."""
    from naive_gpt import ext
    run, tuner = suite.model_step(kind)

    def step(pattern):
        fresh_caches()
        ext.reset_paths()
        if pattern is None:
            outs = run()
            torch.cuda.synchronize()
            state = None
        else:
            with guard.guarded(pattern, band_bytes=65536, skew=skew) as state:
                outs = run()
                torch.cuda.synchronize()
        outs = [o.detach().clone() for o in outs]
        if state is not None:
            _verify(state, '{} step under {}'.format(kind, pattern))
            assert state.allocations > 0 and state.unguarded == 0, (state.allocations, state.unguarded)
            print('guard step {} {}: allocations {} by {} functions'.format(kind, pattern, state.allocations,
                                                                            len(state.sites)))
            state.release()
        return outs, dict(ext.paths_taken())

    try:
        base, paths = step(None)
        for site, want in suite.STEP_PATHS:
            assert _sites(paths, site) == {want}, (site, sorted(paths))
        assert len(base) > 10
        for pattern in guard.PATTERNS:
            outs, taken = step(pattern)
            assert taken == paths, 'the guarded step under {} took different paths'.format(pattern)
            assert len(outs) == len(base)
            for i, (a, b) in enumerate(zip(base, outs)):
                assert torch.isfinite(b).all(), '{}: output {} not finite under {}'.format(kind, i, pattern)
                if not same_bits(a, b):
                    _close(b, a, 'step output {} under {}'.format(i, pattern), rtol=1e-5)
    finally:
        tuner.release()


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_model_step_stays_inside_its_buffers(kind):
    """`_guarded_steps` with every allocation where the allocator would put it (skew 0)."""
    _guarded_steps(kind)
