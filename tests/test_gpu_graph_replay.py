"""Every HIP entry of naive_gpt.ext captured in a HIP graph after a warm warm-up and replayed on
new contents of its input buffers: the replay equals an eager call on them (tests/replay.py).

The cases are those of test_gpu_guard_bands: the poison registry, the d_head-80 attention cases
and the add + norm width cases.  Per case: build A, run it eagerly; capture it; refresh A's
buffers from a second build B with shifted seeds (`full`), or by a transform of the floating
tensors where B does not pair up (`values`); replay; run eagerly on the refreshed buffers; copy
the originals back and replay again.

* the refresh changed at least one output (a case for which it does not shows nothing);
* DET cases: the first replay equals the eager run on the refreshed buffers and the second equals
  the first eager run, in every output, bit for bit;
* ATOMIC cases: the outputs that two eager runs reproduce on both contents are held the same way,
  the others are NaN-free and pass the reference check of the build whose contents they hold;
* a capture that raises is a failure of the entry.

A case named in EXEMPT (none today) would run the same steps as plain calls on a side stream,
caches left warm, and be compared the same way.

Below the entries: a wrapper that is stale on purpose (the protocol must see it), and the blocks
and modules whose host-side memos meet a static input: an upgraded TransformerBlock, its attention
module and one LoRALinear alone, the fused head loss, and the sddmm / spmm autograd operators.
"""
import contextlib
import time

import numpy as np
import pytest
import torch

import replay
import test_gpu_guard_bands as bands
import test_gpu_poisoned_buffers as suite
from poison import fresh_caches, same_bits
from test_gpu_poisoned_buffers import ATOMIC, DET, _close, _sites

pytestmark = pytest.mark.gpu

PARAMS = bands.PARAMS

# (entry, case name) -> why the case cannot be captured, naming the line that forces it.  At most 3;
# none today: no launching wrapper of ext reads device memory on the host.
EXEMPT = {}


@contextlib.contextmanager
def _dev_is(uploads):
    plain, suite._dev = suite._dev, uploads
    try:
        yield
    finally:
        suite._dev = plain


class _Built:
    """One build of a case with `_dev` recorded: `call` runs the build's closure, `inputs()` are
    the device tensors it holds and, once it has run, the masters of what it uploads itself."""

    def __init__(self, case, shifted):
        self.uploads = replay.Uploads()
        with _dev_is(self.uploads), (replay.shifted_seeds(suite) if shifted else contextlib.nullcontext()):
            built = case.build()
        self.raw, self.check = built[0], built[1]
        self.memo = built[2] if len(built) > 2 else ()

    def call(self):
        with _dev_is(self.uploads), self.uploads.running():
            return self.raw()

    def inputs(self):
        found = replay.inputs_of(self.raw)
        found.update(self.uploads.inputs())
        return found


@pytest.mark.parametrize('entry,case', PARAMS)
def test_entry_replayed_on_new_inputs_equals_eager(entry, case):
    from naive_gpt import ext
    ext.load_library()
    what = '{} ({})'.format(entry, case.name)
    started = time.perf_counter()
    a, b = _Built(case, False), _Built(case, True)
    first = a.call()
    torch.cuda.synchronize()
    a.check([o.clone() for o in suite._flatten(first)])
    del first

    def refresh_inputs():
        if a.uploads.masters or case.kind == ATOMIC:      # B's masters, and what B's check learns from its call
            b.call()
            torch.cuda.synchronize()
        return replay.refresh(a.inputs(), b.inputs())

    runs = replay.run(a.call, a.inputs, refresh_inputs, memo=a.memo + b.memo,
                      capture=(entry, case.name) not in EXEMPT, twice=case.kind == ATOMIC, what=what)
    if case.kind == ATOMIC:
        assert runs.mode == 'full', what + ': an ATOMIC case refreshed by values has no reference for its new contents'
    held = replay.compare(runs, case.kind == DET, what, check_refreshed=b.check, check_original=a.check)
    fresh_caches(*a.memo)
    print('replay {}-{}: {} refresh of {} inputs ({} uploaded by the call), {}/{} outputs bitwise, {:.2f} s'.format(
        entry, case.name, runs.mode, len(a.inputs()), len(a.uploads.masters), sum(held), len(held),
        time.perf_counter() - started))


def test_a_launch_the_capture_skipped_is_seen():
    """A wrapper that memoises split_bf16(x) on (id(x), x._version), as a careless cache would: the
    warm-up fills it, the capture hits it, and the graph holds no launch that makes the image.  A
    replay on new contents of x then multiplies the old image (nothing is out of bounds: the
    image stays alive and only holds old values).  The protocol must fail its first comparison."""
    from naive_gpt import ext
    ext.load_library()
    gen = suite._gen(6)
    rows, cols, n = 512, 256, 256         # (a shape that takes the image path: the GEMM reads the image alone)
    x, w = suite._randn(gen, rows, cols), suite._randn(gen, n, cols)
    x_new = suite._randn(gen, rows, cols)
    off = suite._offsets([rows])
    memo = {}

    def stale_image(t):
        key = (id(t), t._version)
        if memo.get('key') != key:
            memo['key'], memo['image'] = key, ext.split_bf16(t)
        return memo['image']

    def call():
        out = ext.grouped_gemm_fused(x, w, off, 1, n=n, k=cols, w_group_stride=n * cols, w_ldn=cols, w_ldk=1,
                                     n_rows=rows, a_image=stale_image(x), w_image=ext.split_bf16(w))
        assert ext.LAST_GEMM_PATH == 'image'
        return out

    runs = replay.run(call, {'x': x}, lambda: replay.refresh({'x': x}, {'x': x_new}), what='stale wrapper')
    assert runs.mode == 'full'
    _close(runs.want1[0], suite._ref_grouped(x_new, w, [rows], n, cols), 'eager on the new x', rtol=1e-5)
    with pytest.raises(AssertionError, match='the capture froze something'):
        replay.compare(runs, True, 'stale wrapper')


# ---------------------------------------------------------------------------------------------------
# blocks and modules on a static input: the memos of ext and of the layers are keyed on the input
# tensor OBJECT and its version, and a static input is the same object at warm-up and capture

# what the attention backward's float atomics (grad_k, grad_v) reach: everything upstream of the
# attention core.  Held to 1e-5 of scale where the bits differ, the bound of
# test_model_step_ignores_what_its_buffers_held for the same reason; every other output bit for bit.
_BEHIND_THE_ATOMICS = ('grad_x', 'mha.linear_q.', 'mha.linear_k.', 'mha.linear_v.', 'mha.attn_fn.', 'norm1.')


def _upgraded_block(kind):
    """The first TransformerBlock of the upgraded model of suite.model_step: STEP_CONFIG dimensions."""
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    torch.manual_seed(0)
    model = utils.upgrade_sparse(checkpoint.build_model(kind, dict(suite.STEP_CONFIG)), d_lora=16).cuda()
    gen = suite._gen(40)
    for name, p in model.named_parameters():
        if name.endswith('lora.right.weight'):          # a fresh adapter is the identity
            p.data.copy_(0.05 * torch.randn(p.shape, generator=gen).cuda())
    return model.decoders[0].train()


def _static(gen, *shape, grad=False):
    return suite._randn(gen, *shape).requires_grad_(grad)


def _step_of(forward, module, x, w):
    """step() -> [y, grad_x, the gradient of every trained parameter], and the outputs' names."""
    trained = [(n, p) for n, p in module.named_parameters() if p.requires_grad]

    def step():
        x.grad = None
        for _, p in trained:
            p.grad = None
        y = forward(x)
        (y * w).sum().backward()
        return [y, x.grad] + [p.grad for _, p in trained]

    def names():
        return ['y', 'grad_x'] + [n for n, p in trained if p.grad is not None]
    return step, names


def _hold(runs, names, loose, what):
    """got1 against want1 and got2 against outs0: the same bits, or, for an output `loose` names,
    within 1e-5 of scale."""
    assert len(names) == len(runs.outs0) == len(runs.got1) == len(runs.want1) == len(runs.got2), what
    assert any(not same_bits(a, b) for a, b in zip(runs.outs0, runs.want1)), what + ': the refresh changed no output'
    for i, name in enumerate(names):
        for got, want, which in ((runs.got1[i], runs.want1[i], 'replay on the refreshed inputs'),
                                 (runs.got2[i], runs.outs0[i], 'replay on the restored inputs')):
            if same_bits(got, want):
                continue
            assert any(name.startswith(p) for p in loose), \
                '{}: {} of the {} differs from the eager run in bits'.format(what, name, which)
            assert torch.isfinite(got).all(), '{}: {} of the {} is not finite'.format(what, name, which)
            _close(got, want, '{}: {} of the {}'.format(what, name, which), rtol=1e-5)


def _tokens():
    return suite.STEP_BATCH, suite.STEP_CONFIG['max_length'], suite.STEP_CONFIG['d_model']


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_upgraded_block_replayed_on_a_new_input(kind):
    """One upgraded TransformerBlock called directly on a static x.requires_grad_(): 2048 tokens,
    d_head 64, N * H = 32 -- the matrix-core attention, the joint q / k / v projection, the fused
    routed FFN, the norm kernels.  The joint projection makes ONE image of its input and hands it to
    its one grouped launch; that image never enters ext's image cache, so this case does not show
    that q / k / v share a CACHED image inside a capture: the `separate` case of
    test_attention_and_a_lone_lora_linear_replayed_on_a_new_input counts those hits."""
    from naive_gpt import ext
    block = _upgraded_block(kind)
    gen = suite._gen(41)
    x, w = _static(gen, *_tokens(), grad=True), _static(gen, *_tokens())
    new = {'x': _static(gen, *_tokens()), 'w': _static(gen, *_tokens())}
    step, names = _step_of(block, block, x, w)
    inputs = {'x': x, 'w': w}
    ext.reset_paths()
    runs = replay.run(step, inputs, lambda: replay.refresh(inputs, new), what=kind + ' block')
    paths = dict(ext.paths_taken())
    for site, want in (('attention', 'mfma'), ('qkv_projection', 'joint'), ('routed_ffn', 'fused'),
                       ('route_topk', 'kernel'), ('norm', 'kernel')):
        assert _sites(paths, site) == {want}, (site, sorted(paths))
    _hold(runs, names(), _BEHIND_THE_ATOMICS, kind + ' block')


@pytest.mark.parametrize('projection', ['joint', 'separate'])
def test_attention_and_a_lone_lora_linear_replayed_on_a_new_input(projection, monkeypatch):
    """The attention module alone, then ONE of its LoRALinears alone on the same static x after an
    eager attention call on it: whatever that call left for (x, version) -- the image of x and, on
    the `separate` path (lora.prepare_shared; here: one adapter table frozen), the down products --
    is warm when the lone layer is warmed up and captured.  On the `separate` path the three
    projections must still share the one image INSIDE the capture."""
    from naive_gpt import ext
    mha = _upgraded_block('opt').mha
    if projection == 'separate':
        mha.linear_v.lora.right.weight.requires_grad_(False)
    gen = suite._gen(42)
    x, w = _static(gen, *_tokens(), grad=True), _static(gen, *_tokens())
    new = {'x': _static(gen, *_tokens()), 'w': _static(gen, *_tokens())}
    inputs = {'x': x, 'w': w}
    served = []
    plain = ext.cached_image

    def counted(*args, **kwargs):
        img = plain(*args, **kwargs)
        served.append((torch.cuda.is_current_stream_capturing(), img is not None))
        return img
    monkeypatch.setattr(ext, 'cached_image', counted)

    step, names = _step_of(lambda t: mha(t, t, t), mha, x, w)
    ext.reset_paths()
    runs = replay.run(step, inputs, lambda: replay.refresh(inputs, new), what=projection + ' attention')
    paths = dict(ext.paths_taken())
    assert _sites(paths, 'attention') == {'mfma'} and _sites(paths, 'qkv_projection') == {projection}, sorted(paths)
    if projection == 'separate':
        assert sum(1 for capturing, hit in served if capturing and hit) >= 3, \
            'q, k and v no longer share one image of x inside a capture: {}'.format(served)
    _hold(runs, names(), ('grad_x', 'linear_q.', 'linear_k.', 'linear_v.', 'attn_fn.'), projection + ' attention')

    lone = mha.linear_q
    step, names = _step_of(lone, lone, x, w)

    def eager_attention():
        with torch.no_grad():
            mha(x, x, x)
    runs = replay.run(step, inputs, lambda: replay.refresh(inputs, new), before=eager_attention,
                      what='a lone LoRALinear after the {} attention'.format(projection))
    _hold(runs, names(), (), 'a lone LoRALinear after the {} attention'.format(projection))


def test_fused_head_loss_replayed_on_a_new_input():
    """layers/tuning/head_loss.py at the smallest fused shape of test_gpu_head_loss, on a static x
    whose image another consumer left in the cache before the warm-up (`cached_image(x2, x)`)."""
    from naive_gpt import ext
    from naive_gpt.layers.tuning import head_loss
    from test_gpu_head_loss import _head
    d, V = 256, 1000
    head = _head(d, V)
    gen = suite._gen(43)

    def targets():
        t = torch.randint(0, V, [4, 512], generator=gen)
        t[0, :7] = -100
        return suite._dev(t)
    x, target = _static(gen, 4, 512, d, grad=True), targets()
    new = {'x': _static(gen, 4, 512, d), 'target': targets()}
    inputs = {'x': x, 'target': target}
    assert head_loss.fused_usable(head, x)
    trained = [head.lora.left.weight, head.lora.right.weight]

    def step():
        x.grad = None
        for p in trained:
            p.grad = None
        loss = head_loss.lm_head_loss(head, x, target)
        (0.37 * loss).backward()
        return [loss, x.grad] + [p.grad for p in trained]

    runs = replay.run(step, inputs, lambda: replay.refresh(inputs, new),
                      before=lambda: ext.image_of(x.detach().reshape(-1, d), x), what='head loss')
    assert runs.mode == 'full'
    _hold(runs, ['loss', 'grad_x', 'grad_left', 'grad_right'], (), 'head loss')


def test_sddmm_and_spmm_operators_replayed_on_a_new_pattern():
    """kernels.sddmm and kernels.spmm, forward and backward, with `indptr` / `indices` the caller
    holds: both backwards take the transposed structure from the memo that ext.transposed_for keeps
    on `indices`.  Refreshed by a full copy from a second ragged pattern of the same shape (the row
    lengths reversed, other columns)."""
    from naive_gpt import kernels
    indptr, idx, q, k, _ = suite._csr_inputs(27)
    B, S, E = q.shape
    gen = suite._gen(44)
    lens = (indptr[1:] - indptr[:-1]).flip(0)
    other = {'indptr': torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(indptr.dtype),
             'indices': torch.randint(0, S, idx.shape, generator=gen, dtype=idx.dtype)}
    assert other['indptr'][-1] == indptr[-1] and not torch.equal(other['indptr'], indptr)
    inputs = {'indptr': suite._dev(indptr), 'indices': suite._dev(idx), 'q': suite._dev(q).requires_grad_(),
              'k': suite._dev(k).requires_grad_(), 'x': _static(gen, B, S, E, grad=True), 'w': _static(gen, B, S, E)}
    new = {'indptr': suite._dev(other['indptr']), 'indices': suite._dev(other['indices']),
           'q': _static(gen, B, S, E), 'k': _static(gen, B, S, E), 'x': _static(gen, B, S, E), 'w': _static(gen, B, S, E)}
    leaves = [inputs[n] for n in ('q', 'k', 'x')]

    def step():
        for t in leaves:
            t.grad = None
        scores = kernels.sddmm(inputs['indptr'], inputs['indices'], inputs['q'], inputs['k'])
        y = kernels.spmm(inputs['indptr'], inputs['indices'], scores, inputs['x'])
        (y * inputs['w']).sum().backward()
        return [scores, y] + [t.grad for t in leaves]

    runs = replay.run(step, inputs, lambda: replay.refresh(inputs, new), memo=(inputs['indices'],),
                      what='sddmm / spmm operators')
    assert runs.mode == 'full'
    _hold(runs, ['scores', 'y', 'grad_q', 'grad_k', 'grad_x'], (), 'sddmm / spmm operators')
