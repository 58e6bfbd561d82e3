"""tests/guard.py itself, on the CPU: the carved tensors equal the plain ones in every property a
wrapper can see, and a write one element outside a tensor is found and named.  These are the
detector's positive controls, so that no GPU test ever has to write out of bounds to show it works.
Every test runs twice: with the tensors' first byte on a 512-byte boundary, and (`*_at_skew_16`) 16
bytes past one, the placement of tests/test_gpu_placement.py."""
import functools

import pytest
import torch

import guard
from guard import guarded, home

BAND = 4096
CPU = dict(band_bytes=BAND, devices=('cpu',), skew=0)      # at_skew_16 below sets the skew for a test


def _make_all():
    """The covered ways to allocate -> {name: tensor}; runs patched or unpatched alike."""
    base = torch.zeros([5, 7]).t()                         # strides (1, 7)
    like = torch.zeros([3], dtype=torch.int32)
    return {
        'list shape': torch.empty([3, 5]),
        'varargs shape': torch.empty(3, 5),
        'empty_like of a transposed tensor': torch.empty_like(base),
        'new_empty': like.new_empty([4, 2]),
        'new_empty with a dtype': like.new_empty([6], dtype=torch.float64),
        'zero elements': torch.empty([0, 8]),
        'bf16 of odd length': torch.empty([33], dtype=torch.bfloat16),
        'int64': torch.empty([9], dtype=torch.int64),
        'uint8 workspace of ragged length': torch.empty([1003], dtype=torch.uint8),
        'bool': torch.empty([5], dtype=torch.bool),
    }


@pytest.mark.parametrize('pattern', guard.PATTERNS)
def test_carved_tensors_look_like_the_plain_ones_and_a_clean_block_verifies(pattern):
    plain = _make_all()
    with guarded(pattern, **CPU) as state:
        carved = _make_all()
        for t in carved.values():
            if t.numel():
                t.fill_(3)                                  # every element of the tensor itself: not a band
    assert torch.empty is state.empty and torch.Tensor.new_empty is state.new_empty     # unpatched again
    assert state.allocations == len(plain) and state.unguarded == 0 and state.homes == 0
    assert state.sites == {'_make_all': len(plain)}
    for name, want in plain.items():
        got = carved[name]
        assert (got.shape, got.dtype, got.stride(), got.device) == (want.shape, want.dtype, want.stride(),
                                                                    want.device), name
        assert got.numel() == 0 or got.data_ptr() % 512 == CPU['skew'], name     # no element: no address
        assert got.is_contiguous() == want.is_contiguous(), name
    storages = [t.untyped_storage().data_ptr() for t in carved.values()]
    assert len(set(storages)) == len(storages), 'one allocation per tensor'
    state.verify()


def _past(t, elements):
    """One element `elements` after t's first (negative: before it), through as_strided."""
    return t.as_strided([1], [1], t.storage_offset() + elements)


def victim(dtype, n=33):
    return torch.empty([n], dtype=dtype)


@pytest.mark.parametrize('pattern', guard.PATTERNS)
@pytest.mark.parametrize('where', ['just past the end', 'just before the start', 'the far end of the trail band'])
def test_one_element_outside_is_found_and_named(pattern, where):
    with guarded(pattern, **CPU) as state:
        other = victim(torch.float32)
        t = victim(torch.bfloat16)                         # 66 bytes: the trail band starts unrounded
    elements = {'just past the end': 33, 'just before the start': -1,
                'the far end of the trail band': 33 + BAND // 2 - 1}[where]
    state.verify()
    _past(t, elements).fill_(2.5)
    with pytest.raises(AssertionError) as err:
        state.verify()
    text = str(err.value)
    assert 'victim allocated' in text and '[33]' in text and 'torch.bfloat16' in text, text
    assert ('lead band' if elements < 0 else 'trail band') in text, text
    assert 'byte offset {} from'.format(2 * elements) in text, text
    assert other is not None


def test_a_store_of_one_is_caught_under_zero_and_missed_under_nan():
    """An int band holds 0 or 1, never a wild index; a stored 1 equals the `nan` pattern.  This is
    why every case runs under both patterns."""
    seen = {}
    for pattern in guard.PATTERNS:
        with guarded(pattern, **CPU) as state:
            t = victim(torch.int32)
        _past(t, 33).fill_(1)
        try:
            state.verify()
            seen[pattern] = 'missed'
        except AssertionError as err:
            assert 'byte offset 132 from' in str(err), str(err)
            seen[pattern] = 'caught'
    assert seen == {'zero': 'caught', 'nan': 'missed'}


def test_band_contents_are_of_the_tensors_own_dtype():
    with guarded('nan', **CPU) as state:
        f, b, i, ws, flag = (victim(d, 5) for d in (torch.float32, torch.bfloat16, torch.int64, torch.uint8,
                                                    torch.bool))
    for t in (f, b):
        around = t.as_strided([BAND // t.element_size() + 5], [1], t.storage_offset())[5:]
        assert torch.isnan(around).all() and torch.isnan(_past(t, -1)).all()
    assert _past(i, 5).item() == 1 and _past(i, -1).item() == 1
    assert _past(flag, 5).item() is True
    # a 5-byte workspace: the 32-bit words counted from its first byte are 1 on either side
    words = ws.as_strided([8], [1], ws.storage_offset() + 8).view(torch.int32)
    assert words.tolist() == [1, 1]
    assert ws.as_strided([4], [1], ws.storage_offset() - 4).view(torch.int32).item() == 1
    assert ws.as_strided([3], [1], ws.storage_offset() + 5).tolist() == [0, 0, 0]
    state.verify()
    with guarded('zero', **CPU) as state:
        f = victim(torch.float32, 5)
    assert (f.as_strided([BAND // 4], [1], f.storage_offset() + 5) == 0).all()
    assert (f.as_strided([BAND // 4], [1], f.storage_offset() - BAND // 4) == 0).all()


@pytest.mark.parametrize('pattern', guard.PATTERNS)
def test_home_keeps_values_dtype_and_shape_and_its_trail_band_starts_at_the_next_byte(pattern):
    with guarded(pattern, **CPU) as state:
        pass
    sources = [torch.arange(35, dtype=torch.float32).view(5, 7).bfloat16(),
               torch.arange(35, dtype=torch.float32).view(5, 7).t(),
               torch.arange(11, dtype=torch.int32),
               torch.zeros([0, 4])]
    for src in sources:
        h = home(src, state, device='cpu')
        assert h.dtype == src.dtype and h.shape == src.shape and h.stride() == src.stride()
        n = src.numel()
        assert torch.equal(h, src)
        assert n == 0 or (h.data_ptr() != src.data_ptr() and h.data_ptr() % 512 == CPU['skew'])
        flat = h.as_strided([n + 1], [1], h.storage_offset())
        band = flat[n:]
        if pattern == 'zero':
            assert band.item() == 0
        else:
            assert torch.isnan(band).all() if src.is_floating_point() else band.item() == 1
    assert state.homes == len(sources) and state.allocations == 0
    assert state.sites == {test_home_keeps_values_dtype_and_shape_and_its_trail_band_starts_at_the_next_byte.__name__:
                           len(sources)}
    state.verify()
    h = home(sources[0], state, caller='somewhere', device='cpu')
    _past(h, 35).fill_(7.0)
    with pytest.raises(AssertionError, match='somewhere allocated.*trail band|trail band.*somewhere allocated'):
        state.verify()


def test_tensors_on_an_unlisted_device_pass_through_untouched():
    with guarded('nan', band_bytes=BAND, devices=('cuda',), skew=CPU['skew']) as state:
        t = torch.empty([4, 4])
        m = torch.empty([4, 4], device='meta')
        like = torch.empty_like(t)
        new = t.new_empty([2])
    assert state.allocations == state.unguarded == state.homes == 0 and not state.blocks
    assert t.storage_offset() == 0 and t.untyped_storage().nbytes() == 64 and m.device.type == 'meta'
    assert like.untyped_storage().nbytes() == 64 and new.untyped_storage().nbytes() == 8


def test_what_cannot_be_rebuilt_is_returned_as_it_is_and_counted():
    with guarded('zero', **CPU) as state:
        s = torch.empty([2, 2], layout=torch.sparse_coo)
        t = torch.empty([2, 2])
    assert s.layout == torch.sparse_coo and s.shape == (2, 2)
    assert state.unguarded == 1 and state.allocations == 1 and t.data_ptr() % 512 == CPU['skew']
    state.verify()


def test_band_bytes_must_be_a_multiple_of_512():
    with pytest.raises(AssertionError):
        with guarded('zero', band_bytes=1000, devices=('cpu',), skew=CPU['skew']):
            pass
    with pytest.raises(AssertionError):
        with guarded('ones', **CPU):
            pass


@pytest.mark.parametrize('skew', [8, 24, -16, 512, 528, 16.0])
def test_skew_must_be_a_multiple_of_16_below_512(skew):
    with pytest.raises(AssertionError, match='skew'):
        with guarded('zero', band_bytes=BAND, devices=('cpu',), skew=skew):
            pass


@pytest.mark.parametrize('skew', [0, 16, 496])
def test_the_first_byte_lies_skew_bytes_past_a_512_byte_boundary(skew):
    """Carved tensors and home() alike, whatever the dtype; the bands still touch the tensor: a store
    one byte before it and one byte after it are both named."""
    with guarded('nan', band_bytes=BAND, devices=('cpu',), skew=skew) as state:
        made = [victim(d, 5) for d in (torch.float32, torch.bfloat16, torch.int32, torch.uint8)]
    made.append(home(torch.arange(35, dtype=torch.float32).view(5, 7).t(), state, device='cpu'))
    assert made[-1].stride() == (1, 7)
    for t in made:
        assert t.data_ptr() % 512 == skew, (t.dtype, t.data_ptr() % 512)
    state.verify()
    b = made[3]                                            # uint8: one element is one byte
    for at, name in ((-1, 'lead band'), (5, 'trail band')):
        keep = _past(b, at).clone()
        _past(b, at).fill_(9)
        with pytest.raises(AssertionError, match=name):
            state.verify()
        _past(b, at).copy_(keep)
        state.verify()


def at_skew_16(test):
    """`test` again with every guarded block of it at skew 16 (through CPU['skew'])."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        CPU['skew'] = 16
        try:
            return test(*args, **kwargs)
        finally:
            CPU['skew'] = 0
    run.__name__ = run.__qualname__ = test.__name__ + '_at_skew_16'
    return run


for _name, _test in sorted(globals().items()):
    if _name.startswith('test_') and callable(_test) and 'skew' not in _name:
        globals()[_name + '_at_skew_16'] = at_skew_16(_test)
