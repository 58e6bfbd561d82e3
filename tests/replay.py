"""Graph replay: make what a capture froze on the host visible.

A replay of a captured HIP graph runs no Python.  Whatever the host decided while the graph was
captured is part of it: a memo hit that skipped a launch, a value read on the host, a pointer taken
out of a cache, a scalar passed by value.  And every buffer the capture allocated has the same
address at every replay and holds what the previous replay left there.  One protocol shows all of
these (`run`, below):

  1. run the closure eagerly on the default stream from empty caches        -> outs0
  2. `captured`: empty the caches, ONE warm-up call on a side stream, then the capture at once,
     nothing cleared in between: the capture meets the caches as the warm-up left them, keyed on
     the very tensor objects and versions it is about to read (what torch's own recipe and
     SparseTuner.capture do)
  3. `refresh` the input buffers in place, replay                            -> got1
  4. empty the caches, run eagerly on the refreshed buffers                  -> want1
  5. copy the saved originals back, replay again                            -> got2

got1 must equal want1 and got2 must equal outs0, bit for bit where the entry is deterministic
(`compare`).  The first catches a launch that is missing from the graph, work that went to another
stream, and a value frozen at capture time; the second catches state that a workspace carries from
one replay into the next.  want1 must differ from outs0, or the refresh has shown nothing.

The inputs of a closure are found in one of two ways, and a case uses the one its builder forces:
`inputs_of` walks the closure's cells (operands the builder uploaded, and what it derived on the
device); a builder that uploads inside its `call` goes through `Uploads` in place of the registry's
`_dev`, which turns each such upload into a device clone of a static master -- a copy from pageable
host memory cannot be captured -- and the masters are the inputs.

What this tier cannot see: a graph with parallel branches (every capture here is one stream, one
chain); steps that span processes; a stale value that happens to equal the fresh one (a memoised
structure refreshed with an equal structure).

One deviation in `refresh`, in both modes: a 0-dim floating tensor is left as it is where a
second build agrees with it in bits ('full'), and always under 'values'.  The scalar this protects
is the upstream gradient `torch.ones([])` of the registry's PQ-loss cases (ATOMIC): their reference
check is `composed_cpu(z, table, 1.0)`, with the 1.0 written out, so a transformed scalar would
fail the check of the outputs that cannot be held bitwise.  Nothing is lost by it: a 0-dim device
tensor can only be frozen into a graph by a host read, and that is a synchronisation, which fails
the capture itself.
"""
import collections
import contextlib
import types

import torch

from poison import fresh_caches, same_bits


# ---------------------------------------------------------------------------------------------------
# the inputs of a closure

def _walk(value, name, found, seen, device_type):
    if id(value) in seen:
        return
    if isinstance(value, torch.Tensor):
        seen.add(id(value))
        if value.device.type == device_type:
            found[name] = value
        return
    if isinstance(value, (str, bytes, int, float, bool, type(None), types.ModuleType, type)):
        return
    seen.add(id(value))
    if isinstance(value, (tuple, list)):
        for i, v in enumerate(value):
            _walk(v, '{}[{}]'.format(name, i), found, seen, device_type)
    elif isinstance(value, dict):
        for k, v in value.items():
            _walk(v, '{}[{!r}]'.format(name, k), found, seen, device_type)
    elif isinstance(value, types.FunctionType):
        for var, cell in zip(value.__code__.co_freevars, value.__closure__ or ()):
            try:
                inner = cell.cell_contents
            except ValueError:          # a cell that is not filled yet
                continue
            _walk(inner, '{}.{}'.format(name, var) if name else var, found, seen, device_type)
    elif isinstance(value, torch.nn.Module):
        for k, v in list(value.named_parameters()) + list(value.named_buffers()):
            _walk(v, '{}.{}'.format(name, k), found, seen, device_type)
    elif hasattr(value, 'buffer'):      # ext.MfmaTiles, ext.SplitImage
        _walk(value.buffer, name + '.buffer', found, seen, device_type)


def inputs_of(call, device_type='cuda') -> 'collections.OrderedDict[str, torch.Tensor]':
    """Every tensor on `device_type` that the closure `call` holds, name -> tensor, in the order of
    `call.__code__.co_freevars` and, inside a cell, of the container: tuples, lists, dicts, nested
    functions' own cells, modules' parameters and buffers, and objects with a `.buffer`.  A tensor
    reachable twice is named once, by the first path."""
    found = collections.OrderedDict()
    _walk(call, '', found, set(), device_type)
    return found


class Uploads:
    """Stands in for the registry's `_dev`.  Outside `running()` (while a case is built) it uploads
    as `_dev` does.  Inside, the n-th host tensor of a call is uploaded once, by the first call,
    into a static master, and every call gets a device clone of the n-th master: a clone is
    captured, and a replay reads the master's contents of that moment.  A tensor already on the
    device is returned as it is, as `.cuda()` returns it."""

    def __init__(self, device='cuda'):
        self.device, self.masters, self._cursor = device, [], None

    def __call__(self, t):
        if t.device.type == torch.device(self.device).type:
            return t
        if self._cursor is None:
            return t.to(self.device)
        i, self._cursor = self._cursor, self._cursor + 1
        if i == len(self.masters):
            assert self.device != 'cuda' or not torch.cuda.is_current_stream_capturing(), \
                'the first call of a closure that uploads must be eager'
            self.masters.append(t.to(self.device))
        m = self.masters[i]
        assert m.shape == t.shape and m.dtype == t.dtype, 'upload {} changed between calls'.format(i)
        return m.clone()

    @contextlib.contextmanager
    def running(self):
        self._cursor = 0
        try:
            yield
        finally:
            self._cursor = None

    def wrap(self, call):
        def wrapped():
            with self.running():
                return call()
        return wrapped

    def inputs(self):
        return collections.OrderedDict(('upload[{}]'.format(i), m) for i, m in enumerate(self.masters))


@contextlib.contextmanager
def shifted_seeds(suite, shift=1000):
    """The registry's `_gen` shifted by `shift`, and its `_once` recomputing (a reference shared by
    the builds of a case belongs to the unshifted seeds), for the duration of the second build."""
    gen, once = suite._gen, suite._once
    suite._gen = lambda s: torch.Generator().manual_seed(s + shift)
    suite._once = lambda memo, make: make()
    try:
        yield
    finally:
        suite._gen, suite._once = gen, once


# ---------------------------------------------------------------------------------------------------
# changing the inputs' contents

def _transform(t):
    """t <- (-0.75 t) rolled by one along dim 0: other bits in every element that is not 0 already
    (those change sign), other values in other places, finite where t was."""
    t.copy_((-0.75 * t).roll(1, 0))


def pairs_up(a_inputs, b_inputs) -> bool:
    return list(a_inputs) == list(b_inputs) and all(
        a.shape == b_inputs[k].shape and a.dtype == b_inputs[k].dtype for k, a in a_inputs.items())


def refresh(a_inputs, b_inputs) -> str:
    """Change the contents of A's buffers in place; neither addresses nor objects change.

    'full': every tensor of A has a partner of the same name, shape and dtype in B (a second,
    valid build of the same case): `a.copy_(b)` for all of them, integers included.  A floating
    pair whose bits agree (the builder took it from no seed) gets the transform of 'values',
    except a 0-dim one, which is left alone (the module docstring says why).
    'values' otherwise: integer and bool tensors are left alone, every floating tensor t of at
    least one dimension becomes (-0.75 t).roll(1, 0).  No integer is ever written that did not come from a valid build."""
    with torch.no_grad():
        if b_inputs is not None and pairs_up(a_inputs, b_inputs):
            for k, a in a_inputs.items():
                b = b_inputs[k]
                if a.is_floating_point() and same_bits(a, b):
                    if a.dim() > 0:
                        _transform(a)
                else:
                    a.copy_(b)
            return 'full'
        for a in a_inputs.values():
            if a.is_floating_point() and a.dim() > 0:
                _transform(a)
        return 'values'


def saved(inputs):
    return collections.OrderedDict((k, t.detach().clone()) for k, t in inputs.items())


def restore(inputs, originals):
    with torch.no_grad():
        for k, t in inputs.items():
            t.copy_(originals[k])


# ---------------------------------------------------------------------------------------------------
# capture and the protocol

def _flatten(outs):
    import test_gpu_poisoned_buffers as suite
    return suite._flatten(outs)


def _on_side_stream(call):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs = call()
    torch.cuda.current_stream().wait_stream(side)
    return outs


def _memo_entries():
    """What the identity-keyed memos hold right now.  Should a capture have taken an address out of
    one of them, a replay reads that address: it must stay allocated until the case ends, so that a
    stale read is a wrong value for the comparison to find and never a memory error."""
    from naive_gpt import ext
    return [memo.values() for memo in ext.MEMOS.values()]


def captured(call, memo=(), before=None):
    """-> (graph, the flattened static outputs, what must stay alive as long as the graph).
    Empty caches, one warm-up call on a side stream, the capture immediately afterwards: no cache
    is cleared in between.  `before()`: eager work on the same tensors in front of the warm-up
    (another consumer of the input, whose by-products the caches then hold).  An exception inside
    the capture propagates."""
    from naive_gpt import ext
    fresh_caches(*memo)
    if before is not None:
        _on_side_stream(before)
    warm = _on_side_stream(call)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = call()
    return graph, _flatten(outs), (warm, outs, ext.held_by_caches(), _memo_entries())


Runs = collections.namedtuple('Runs', 'outs0 outs0_again got1 want1 want1_again got2 mode')


def _eager(call, memo):
    fresh_caches(*memo)
    outs = call()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in _flatten(outs)]


def run(call, inputs, refresh_inputs, memo=(), capture=True, twice=False, what='', before=None) -> Runs:
    """The protocol of the module docstring on `call`, whose device inputs are `inputs` (a mapping,
    or a function that returns it once `call` has run);
    `refresh_inputs()` changes them in place and returns the mode.  `twice`: every eager run is
    made twice (what reproduces is decided from the pairs).  `capture=False`: the replays are
    plain calls on a side stream after a warm-up call there, caches left as they are: what an
    entry that cannot be captured is still held to.  `before`: see `captured`; the eager runs start
    from empty caches without it."""
    outs0 = _eager(call, memo)
    outs0_again = _eager(call, memo) if twice else outs0
    if capture:
        try:
            graph, static, keep = captured(call, memo, before)
        except Exception as err:
            torch.cuda.synchronize()
            raise AssertionError('{}: the capture raised {}: {}'.format(what, type(err).__name__, err)) from err

        def replay():
            graph.replay()
            torch.cuda.synchronize()
            return [o.detach().clone() for o in static]
    else:
        fresh_caches(*memo)
        if before is not None:
            _on_side_stream(before)
        keep = _on_side_stream(call)

        def replay():
            outs = _on_side_stream(call)
            torch.cuda.synchronize()
            return [o.detach().clone() for o in _flatten(outs)]
    if callable(inputs):            # (a closure that uploads has its masters after its first call)
        inputs = inputs()
    originals = saved(inputs)
    mode = refresh_inputs()
    got1 = replay()
    want1 = _eager(call, memo)
    want1_again = _eager(call, memo) if twice else want1
    fresh_caches(*memo)
    restore(inputs, originals)
    got2 = replay()
    del keep
    return Runs(outs0, outs0_again, got1, want1, want1_again, got2, mode)


def _nan_free(outs, what):
    for i, o in enumerate(outs):
        assert not (o.is_floating_point() and torch.isnan(o).any()), '{}: NaN in output {}'.format(what, i)


def compare(runs: Runs, deterministic: bool, what: str, check_refreshed=None, check_original=None):
    """The assertions of the tier on what `run` returned.  Deterministic: every output in the same
    bits.  Otherwise (float atomics in no fixed order): the outputs that both pairs of eager runs
    reproduce are held bitwise, the others are NaN-free and pass the case's own checks."""
    n = len(runs.outs0)
    assert n > 0 and all(len(r) == n for r in runs[:6]), what + ': the runs differ in their number of outputs'
    assert any(not same_bits(a, b) for a, b in zip(runs.outs0, runs.want1)), \
        what + ': the refresh ({}) changed no output: the case shows nothing'.format(runs.mode)
    if deterministic:
        held = [True] * n
    else:
        held = [same_bits(runs.outs0[i], runs.outs0_again[i]) and same_bits(runs.want1[i], runs.want1_again[i])
                for i in range(n)]
    for i in range(n):
        if not held[i]:
            continue
        assert same_bits(runs.got1[i], runs.want1[i]), \
            '{}: output {} of the replay on refreshed inputs ({}) differs from the eager run on them: ' \
            'the capture froze something'.format(what, i, runs.mode)
        assert same_bits(runs.got2[i], runs.outs0[i]), \
            '{}: output {} of the replay on the restored inputs differs from the first eager run: ' \
            'state carried from one replay to the next'.format(what, i)
    if not all(held):
        _nan_free(runs.got1, what + ' (refreshed)')
        _nan_free(runs.got2, what + ' (restored)')
        if check_refreshed is not None:
            check_refreshed(runs.got1)
        if check_original is not None:
            check_original(runs.got2)
    return held
