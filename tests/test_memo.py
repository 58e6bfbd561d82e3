"""`ext._Stamped`, the one type behind every host-side memo, held to its rule on CPU
tensors with `ext.capture_tag` played by hand and its calls counted: 0 is eager code, 5 and 6 are two
captures."""
import gc

import pytest
import torch

from naive_gpt import ext
from naive_gpt.layers.tuning import lora
from poison import fresh_caches

AT = torch.zeros(1)               # the tensor whose device's stream a memo asks about
SHARED = ext.MEMOS['lora.shared']          # (layers/tuning/lora.py: prepare_shared)


@pytest.fixture
def tag(monkeypatch):
    """[the tag now, how often it was asked]"""
    state = [0, 0]

    def played(dev=None):
        state[1] += 1
        return state[0]

    monkeypatch.setattr(ext, 'capture_tag', played)
    ext.clear_memos()
    yield state
    ext.clear_memos()


def _asked(tag):
    asked, tag[1] = tag[1], 0
    return asked


def test_an_entry_is_served_only_under_the_tag_it_was_made_with(tag):
    memo = ext._Stamped()
    x = torch.zeros([4, 32])
    for made in (0, 5, 6):
        tag[0] = made
        memo.keep(x, ('s',), 'made under {}'.format(made), AT)
        for asked in (0, 5, 6):
            tag[0] = asked
            assert memo.find(x, ('s',), AT) == (('made under {}'.format(made) if asked == made else None), asked)


def test_stamp_version_and_identity(tag):
    memo = ext._Stamped()
    x = torch.zeros([4, 32])
    memo.keep(x, (x._version, 64), 'value', AT)
    assert memo.find(x, (x._version, 64), AT)[0] == 'value'
    assert memo.find(x, (x._version, 80), AT) == (None, None), 'another stamp was served'
    x.add_(1)
    assert memo.find(x, (x._version, 64), AT) == (None, None), 'an in-place write to the owner went unseen'
    memo.keep(x, (x._version, 64), 'value', AT)
    twin = torch.zeros([4, 32])
    assert memo.find(twin, (twin._version, 64), AT) == (None, None)
    assert memo.find(x.view(4, 32), (x._version, 64), AT) == (None, None), 'a view is another object'
    # an address handed on: whatever object comes after the owner, at its `id` or elsewhere, finds nothing
    stamp = (x._version, 64)
    del x
    gc.collect()
    assert memo.values() == [] and not memo.data, 'the weak reference\'s callback removes the entry'
    later = [torch.zeros([4, 32]) for _ in range(8)]
    assert all(memo.find(t, stamp, AT) == (None, None) for t in later)


def test_an_entry_under_the_id_of_another_object_is_not_served(tag):
    """The identity test itself, with the callback's work undone by hand: an entry that sits under the
    `id` of a tensor it was not made for is a miss, while its owner lives and after it died."""
    memo = ext._Stamped()
    x, other = torch.zeros(3), torch.zeros(3)
    memo.keep(other, ('s',), 'of another tensor', AT)
    memo.data[id(x)] = memo.data.pop(id(other))
    assert memo.find(x, ('s',), AT) == (None, None)
    del other
    gc.collect()
    assert memo.values() == ['of another tensor'] and memo.find(x, ('s',), AT) == (None, None)
    assert _asked(tag) == 1, 'only the `keep` asks'


def test_the_bound_evicts_the_least_recently_used(tag):
    bound = [2]
    memo = ext._Stamped(bound=lambda: bound[0])
    a, b, c, d = (torch.zeros(2) for _ in range(4))
    memo.keep(a, (), 'a', AT)
    memo.keep(b, (), 'b', AT)
    assert memo.find(a, (), AT)[0] == 'a'                  # a hit refreshes: b is now the oldest
    memo.keep(c, (), 'c', AT)
    assert memo.values() == ['a', 'c'] and memo.find(b, (), AT) == (None, None)
    memo.keep(a, (), 'a again', AT)                        # so does keeping
    memo.keep(d, (), 'd', AT)
    assert memo.values() == ['a again', 'd']
    bound[0] = 1                                            # (read at the call, as IMAGE_CACHE_ENTRIES is)
    memo.keep(b, (), 'b', AT)
    assert memo.values() == ['b']
    memo.clear()
    assert memo.values() == []


def test_image_cache_keeps_image_cache_entries(tag, monkeypatch):
    xs = [torch.zeros([4, 32]) for _ in range(3)]
    for i, x in enumerate(xs):
        ext.put_image(x, None, i)
    assert [ext.cached_image(x) for x in xs] == [None, 1, 2]
    monkeypatch.setattr(ext, 'IMAGE_CACHE_ENTRIES', 3)
    ext.put_image(xs[0], xs[0], 0)
    assert [ext.cached_image(x) for x in xs] == [0, 1, 2]


def test_frozen_exception(tag):
    memo = ext._Stamped(frozen_from_eager=True)
    plain = ext._Stamped()
    frozen, trained = torch.zeros(3), torch.zeros(3, requires_grad=True)
    for m in (memo, plain):
        m.keep(frozen, (), 'frozen, eager', AT)
        m.keep(trained, (), 'trained, eager', AT)
    for inside in (5, 6):
        tag[0] = inside
        assert memo.find(frozen, (), AT) == ('frozen, eager', inside)
        assert memo.find(trained, (), AT) == (None, inside)
        assert plain.find(frozen, (), AT) == (None, inside), 'the exception is an option, not the rule'
    tag[0] = 5
    memo.keep(frozen, (), 'frozen, capture 5', AT)
    for other in (0, 6):
        tag[0] = other
        assert memo.find(frozen, (), AT) == (None, other), 'a capture\'s entry was served outside it'
    per_parameter = ext._PerParameter()
    assert per_parameter.frozen_from_eager and not ext.MEMOS['images'].frozen_from_eager
    assert not ext._TRANSPOSED.frozen_from_eager and not SHARED.frozen_from_eager
    assert ext._WEIGHT_IMAGES.frozen_from_eager and ext._WEIGHT_NORMS.frozen_from_eager


def test_the_tag_is_asked_exactly_when_the_rule_says(tag, monkeypatch):
    memo = ext._Stamped()
    x, y = torch.zeros([4, 32]), torch.zeros([4, 32])
    memo.keep(x, (0,), 'value', AT)
    assert _asked(tag) == 1, 'a keep with no answer handed to it asks once'
    memo.keep(x, (0,), 'value', AT, tag=0)
    assert _asked(tag) == 0, 'a keep that was handed the lookup\'s answer asks nothing'
    assert memo.find(y, (0,), AT) == (None, None) and _asked(tag) == 0, 'a miss on identity asked'
    assert memo.find(x, (1,), AT) == (None, None) and _asked(tag) == 0, 'a miss on the stamp asked'
    assert memo.find(x, (0,), AT) == ('value', 0) and _asked(tag) == 1
    tag[0] = 5
    assert memo.find(x, (0,), AT) == (None, 5) and _asked(tag) == 1, 'a would-be hit asks once'

    # the callers: the lone layers of an eager step ask nothing; a rebuild reuses the lookup's answer
    built = []
    monkeypatch.setattr(ext, 'split_bf16', lambda t: built.append('image') or ('image', len(built)))
    monkeypatch.setattr(ext, 'csr_transpose', lambda indptr, indices, d_head=64: built.append('csr') or ('csr', len(built)))
    tag[0] = 0
    assert ext.cached_image(x) is None and _asked(tag) == 0
    first = ext.image_of(x)
    assert _asked(tag) == 1 and ext.image_of(x) is first and ext.cached_image(x) is first and _asked(tag) == 2
    tag[0] = 5
    assert ext.image_of(x) is not first and _asked(tag) == 1, 'would-be hit, wrong tag, rebuild: one query in all'
    ext.put_image(x, x, 'handed in')
    assert _asked(tag) == 1
    indptr, indices = torch.zeros(3, dtype=torch.int32), torch.zeros([1, 4], dtype=torch.int32)
    eager = ext.transposed_for(indptr, indices)
    assert _asked(tag) == 1 and ext.transposed_for(indptr, indices) is eager and _asked(tag) == 1
    tag[0] = 6
    assert ext.transposed_for(indptr, indices) is not eager and _asked(tag) == 1
    assert ext.transposed_for(indptr, indices, 80) is not None and _asked(tag) == 1, 'another head size: a make'
    w = torch.zeros([4, 32])
    tag[0] = 0
    norms = ext.weight_row_norms(w)
    assert _asked(tag) == 1 and ext.weight_row_norms(w) is norms and _asked(tag) == 1
    assert built == ['image', 'image', 'csr', 'csr', 'csr']


def test_inference_tensors_bypass_the_memos(tag, monkeypatch):
    monkeypatch.setattr(ext, 'split_bf16', lambda t: ['image'])
    with torch.inference_mode():
        x = torch.zeros([4, 32])
    assert ext.image_of(x) is not ext.image_of(x) and ext.cached_image(x) is None
    ext.put_image(x, x, 'handed in')
    assert ext.weight_row_norms(x) is not ext.weight_row_norms(x)
    assert lora._shared_u(x, torch.zeros(3)) is None
    assert all(memo.values() == [] for memo in ext.MEMOS.values()) and tag[1] == 0


def _fill_every_memo():
    """One entry in every registered memo, whatever registers later included."""
    owners = [torch.zeros([4, 32]) for _ in ext.MEMOS]
    for memo, owner in zip(ext.MEMOS.values(), owners):
        memo.keep(owner, (owner._version,), torch.zeros(1), AT)
    assert all(len(memo.values()) == 1 for memo in ext.MEMOS.values())
    return owners


def test_registry(tag):
    assert {'images', 'transposed', 'weight_images', 'weight_norms', 'lora.shared'} <= set(ext.MEMOS)
    assert ext._Stamped() not in ext.MEMOS.values(), 'a nameless memo belongs to whoever made it'
    owners = _fill_every_memo()
    assert ext.held_by_caches() == ext._WEIGHT_IMAGES.values() + ext._WEIGHT_NORMS.values()
    assert len(ext.held_by_caches()) == 2
    shared, transposed = SHARED.values(), ext._TRANSPOSED.values()
    ext.drop_images()
    for name, memo in ext.MEMOS.items():
        assert (memo.values() == []) == (name in ('images', 'weight_images', 'weight_norms')), name
    assert SHARED.values() == shared and ext._TRANSPOSED.values() == transposed
    assert ext.held_by_caches() == []
    ext.clear_memos()
    assert all(memo.values() == [] for memo in ext.MEMOS.values())
    del owners


def test_fresh_caches_empties_every_registered_memo(tag):
    owners = _fill_every_memo()
    late = ext._Stamped('registered by a test')
    try:
        late.keep(owners[0], (), 'value', AT)
        fresh_caches()
        assert all(memo.values() == [] for memo in ext.MEMOS.values()) and late.values() == []
    finally:
        del ext.MEMOS['registered by a test']
