"""The graph-replay tier runs exactly the cases of the guard-band tier (so its coverage of ext's
entries is the poison registry's, which test_poison_coverage holds complete), and its exemptions
are few (none today), real and explained."""
import test_gpu_graph_replay as tier
import test_gpu_guard_bands as bands


def _ids(params):
    return [p.id for p in params]


def test_the_parametrisation_is_that_of_the_guard_band_tier():
    assert _ids(tier.PARAMS) == _ids(bands.PARAMS)
    assert [p.values for p in tier.PARAMS] == [p.values for p in bands.PARAMS]
    assert len(set(_ids(tier.PARAMS))) == len(tier.PARAMS) > 80
    marks = [m for m in tier.test_entry_replayed_on_new_inputs_equals_eager.pytestmark if m.name == 'parametrize']
    assert len(marks) == 1 and marks[0].args[1] is tier.PARAMS


def test_exemptions_are_few_named_and_explained():
    assert len(tier.EXEMPT) <= 3
    cases = {(p.values[0], p.values[1].name) for p in tier.PARAMS}
    for key, reason in tier.EXEMPT.items():
        assert key in cases, '{} is exempt but is no case of the tier'.format(key)
        assert isinstance(reason, str) and len(reason.strip()) > 40, key
        assert '.py' in reason, '{}: the reason names no line of code'.format(key)
