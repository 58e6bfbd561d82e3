"""tests/replay.py on CPU tensors: what `inputs_of` finds and in which order, when two builds pair
up, what `refresh` writes in either mode, that saved clones restore exactly, and whom ext's memos
serve under which capture tag."""
import torch

import replay
from poison import same_bits


class _Image:
    def __init__(self, buffer):
        self.buffer = buffer


def _build(seed, rows=5, extra_row=False):
    """A builder in the registry's style: operands in cells, in a list, a dict, an object with a
    `.buffer`, a module, and behind a nested function."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn([rows + (1 if extra_row else 0), 4], generator=gen)
    pair = [torch.randn([rows, 3], generator=gen), torch.randint(0, rows, [rows], generator=gen, dtype=torch.int32)]
    named = {'scale': torch.rand([rows], generator=gen), 'mask': torch.rand([rows], generator=gen) > 0.5}
    image = _Image(torch.randn([16], generator=gen).bfloat16())
    module = torch.nn.Linear(3, 2)
    constant = torch.full([rows, 2], 1.5)       # from no seed: the same in every build
    scalar = torch.ones([])
    count = 7

    def inner():
        return constant * count

    def call():
        return a[:rows].sum() + pair[0][pair[1].long()].sum() + named['scale'].sum() + named['mask'].sum() \
            + image.buffer.float().sum() + module.weight.sum() + inner().sum() + scalar

    return call


NAMES = ['a', 'image.buffer', 'inner.constant', 'module.weight', 'module.bias', 'named[\'scale\']', 'named[\'mask\']',
         'pair[0]', 'pair[1]', 'scalar']


def test_inputs_of_finds_nested_tensors_in_a_stable_order():
    found = replay.inputs_of(_build(0), device_type='cpu')
    assert list(found) == NAMES
    assert list(replay.inputs_of(_build(1), device_type='cpu')) == NAMES
    assert found['pair[1]'].dtype == torch.int32 and found['image.buffer'].dtype == torch.bfloat16
    assert not replay.inputs_of(_build(0), device_type='cuda')


def test_a_tensor_reachable_twice_is_named_once():
    t = torch.zeros(3)
    both = [t, (t,)]

    def call():
        return t, both
    assert list(replay.inputs_of(call, device_type='cpu')) == ['both[0]']


def test_two_builds_pair_up_unless_a_shape_differs():
    a = replay.inputs_of(_build(0), device_type='cpu')
    assert replay.pairs_up(a, replay.inputs_of(_build(1000), device_type='cpu'))
    assert not replay.pairs_up(a, replay.inputs_of(_build(1000, extra_row=True), device_type='cpu'))
    fewer = replay.inputs_of(_build(1000), device_type='cpu')
    del fewer['scalar']
    assert not replay.pairs_up(a, fewer)


def test_full_refresh_copies_everything_and_restores_exactly():
    a = replay.inputs_of(_build(0), device_type='cpu')
    b = replay.inputs_of(_build(1000), device_type='cpu')
    ptrs = {k: t.data_ptr() for k, t in a.items()}
    before = replay.saved(a)
    constant = a['inner.constant'].clone()
    assert replay.refresh(a, b) == 'full'
    assert {k: t.data_ptr() for k, t in a.items()} == ptrs, 'a refresh writes in place'
    for k in NAMES:
        if k in ('inner.constant', 'scalar'):
            continue
        assert same_bits(a[k], b[k]), k
    assert not same_bits(a['pair[1]'], before['pair[1]']), 'the structure changes too'
    # identical in both builds: the transform, except for the 0-dim scalar (replay.py says which one it protects)
    assert same_bits(a['inner.constant'], (-0.75 * constant).roll(1, 0))
    assert same_bits(a['scalar'], torch.ones([]))
    for k in NAMES:
        if k != 'scalar' and a[k].is_floating_point():
            assert not same_bits(a[k], before[k]), k + ' did not change'
    replay.restore(a, before)
    for k in NAMES:
        assert same_bits(a[k], before[k]), k


def test_values_refresh_leaves_integers_and_changes_every_float():
    a = replay.inputs_of(_build(0), device_type='cpu')
    b = replay.inputs_of(_build(1000, extra_row=True), device_type='cpu')
    before = replay.saved(a)
    assert replay.refresh(a, b) == 'values'
    assert replay.refresh(dict(a), None) == 'values'
    replay.restore(a, before)
    assert replay.refresh(a, b) == 'values'
    for k in NAMES:
        if a[k].is_floating_point() and a[k].dim() > 0:
            assert same_bits(a[k], (-0.75 * before[k]).roll(1, 0)), k
            assert not same_bits(a[k], before[k]), k + ' did not change'
        else:
            assert same_bits(a[k], before[k]), k + ': an integer or bool tensor was written'
    replay.restore(a, before)
    assert all(same_bits(a[k], before[k]) for k in NAMES)


def test_the_transform_changes_the_bits_of_zeros_and_ones_too():
    for t in (torch.zeros([4, 2]), torch.ones([1]), torch.ones([3]).bfloat16()):
        before = t.clone()
        replay.refresh({'t': t}, None)
        assert not same_bits(t, before) and torch.isfinite(t).all()


def test_uploads_inside_a_call_become_clones_of_static_masters():
    up = replay.Uploads(device='meta')          # any device the host tensors are not on
    host = torch.arange(6.0)
    assert up(host).device.type == 'meta' and not up.masters, 'outside a call: a plain upload'
    first, second = [], []
    for sink in (first, second):
        with up.running():
            sink += [up(host), up(host[:2])]
    assert len(up.masters) == 2 and list(up.inputs()) == ['upload[0]', 'upload[1]']
    assert first[0] is not up.masters[0] and second[0] is not first[0]
    assert second[1].shape == (2,)
    on_device = torch.empty([3], device='meta')
    assert up(on_device) is on_device


def test_shifted_seeds_shift_and_put_back():
    import test_gpu_poisoned_buffers as suite
    gen, once = suite._gen, suite._once
    plain = torch.rand([3], generator=suite._gen(5))
    with replay.shifted_seeds(suite):
        assert torch.equal(torch.rand([3], generator=suite._gen(5)), torch.rand([3], generator=gen(1005)))
        memo = {'value': 1}
        assert suite._once(memo, lambda: 2) == 2, 'a shared reference belongs to the unshifted seeds'
    assert suite._gen is gen and suite._once is once
    assert torch.equal(torch.rand([3], generator=suite._gen(5)), plain)


def test_memo_entries_are_served_only_under_the_capture_tag_they_were_made_with(monkeypatch):
    """The host side of ext's memos with `capture_tag` played by hand: 0 is eager code, 5 and 6 are
    two captures."""
    from naive_gpt import ext
    tag = [0]
    monkeypatch.setattr(ext, 'capture_tag', lambda dev=None: tag[0])
    ext.drop_images()
    try:
        x = torch.zeros([4, 32])
        ext.put_image(x, x, 'eager image')
        assert ext.cached_image(x, x) == 'eager image'
        tag[0] = 5
        assert ext.cached_image(x, x) is None, 'an image made by eager code was served inside a capture'
        ext.put_image(x, x, 'image of capture 5')
        assert ext.cached_image(x, x) == 'image of capture 5', 'q, k and v share one image inside a capture'
        tag[0] = 6
        assert ext.cached_image(x, x) is None, 'an image of one capture was served inside another'
        tag[0] = 0
        assert ext.cached_image(x, x) is None, 'an image in a graph\'s pool was served to eager code'

        cache = ext._PerParameter()
        frozen, trained = torch.zeros(3), torch.zeros(3, requires_grad=True)
        cache.put(frozen, 'frozen, eager')
        cache.put(trained, 'trained, eager')
        assert cache.get(frozen) == 'frozen, eager' and cache.get(trained) == 'trained, eager'
        tag[0] = 5
        assert cache.get(frozen) == 'frozen, eager', 'nothing in a captured step writes a frozen weight'
        assert cache.get(trained) is None, 'a trained weight\'s eager by-product was served inside a capture'
        cache.put(trained, 'trained, capture 5')
        assert cache.get(trained) == 'trained, capture 5'
        tag[0] = 6
        assert cache.get(trained) is None
        tag[0] = 0
        assert cache.get(trained) is None and cache.get(frozen) == 'frozen, eager'
        with torch.no_grad():
            frozen.add_(1)
        assert cache.get(frozen) is None, 'the version counter still drops an entry'
    finally:
        ext.drop_images()


def test_image_of_and_transposed_for_rebuild_across_a_capture_boundary(monkeypatch):
    """`image_of` and `transposed_for` with the launches behind them counted and `capture_tag`
    played by hand: one build per tag, shared within it."""
    from naive_gpt import ext
    tag, built = [0], []
    monkeypatch.setattr(ext, 'capture_tag', lambda dev=None: tag[0])
    monkeypatch.setattr(ext, 'split_bf16', lambda x: built.append('image') or ('image', len(built)))
    monkeypatch.setattr(ext, 'csr_transpose', lambda indptr, indices, d_head=64: built.append('csr') or ('csr', len(built)))
    ext.drop_images()
    try:
        x = torch.zeros([4, 32])
        first = ext.image_of(x)
        assert ext.image_of(x) is first and built == ['image']
        tag[0] = 5
        inside = ext.image_of(x)
        assert inside is not first and ext.image_of(x) is inside and ext.cached_image(x) is inside
        tag[0] = 0
        assert ext.cached_image(x) is None and ext.image_of(x) is not inside and built == ['image'] * 3
        indptr, indices = torch.zeros(3, dtype=torch.int32), torch.zeros([1, 4], dtype=torch.int32)
        eager = ext.transposed_for(indptr, indices)
        assert ext.transposed_for(indptr, indices) is eager
        tag[0] = 6
        captured = ext.transposed_for(indptr, indices)
        assert captured is not eager and ext.transposed_for(indptr, indices) is captured
        tag[0] = 0
        assert ext.transposed_for(indptr, indices) is not captured
        assert built.count('csr') == 3
    finally:
        ext.drop_images()
