"""Grouped key/value heads (GQA / MQA) at the C ABI, checked without a GPU: the new entries are
declared, exported and bound, the ABI version did not move, and every precondition include/spt_hip.h
states for them is refused with the stated code before anything touches the device.

The refusal rows follow test_contract_refusals.py: made-up non-NULL device addresses, one violated
condition per row, and only where no GPU is visible (there a call that gets past its validation
returns HIP's "no device" error, a positive code, and can harm nothing)."""
import ctypes

import pytest

import test_abi
import test_contract_refusals as R

NEW = ('spt_attention_mfma_forward_kv', 'spt_attention_mfma_backward_kv', 'spt_lookup_forward_kv',
       'spt_head_group_sum')
SPT_EINVAL, SPT_ESHAPE = R.SPT_EINVAL, R.SPT_ESHAPE

# calls that get past every precondition: N = 2 samples of 6 query heads, 2 kv heads, S = 64, Z = 8
ATTN = dict(layout=0, batch_size=12, seq_length=64, d_head=64, nnz=64 * 8, scale=0.125, clamp=10.0, heads=6,
            kv_heads=2)
BASE = {
    'spt_attention_mfma_forward_kv': dict(ATTN, y_transposed=0),
    'spt_attention_mfma_backward_kv': dict(ATTN, transposed=0),
    'spt_lookup_forward_kv': dict(batch_size=12, seq_length=128, n_subspaces=8, sparsity=8, heads=6, kv_heads=2),
    'spt_head_group_sum': dict(rows=128, heads=6, kv_heads=2, d_head=64),
}
# pointers that may be NULL
OPTIONAL = {'bounds', 'stream'}


def _call(lib, entry, **changes):
    values = dict(BASE[entry])
    values.update(changes)
    args, keep = R._bind(lib, entry, values)
    return getattr(lib, entry)(*args)


@pytest.fixture(scope='module')
def lib():
    from naive_gpt import ext
    return ext.load_library()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from naive_gpt import ext
    declared = test_abi.declared_symbols()
    protos = R.prototypes()
    raw = ctypes.CDLL(test_abi.LIB)
    for name in NEW:
        assert name in declared, name + ' is not in include/spt_hip.h'
        assert hasattr(raw, name), name + ' is not exported'
        assert name in ext._PROTOTYPES, name + ' is not bound'
        assert len(ext._PROTOTYPES[name][0]) == len(protos[name]), name
        assert getattr(lib, name).restype is ctypes.c_int


def test_abi_version_is_still_40(lib):
    from naive_gpt import ext
    assert lib.spt_abi_version() == 40 and ext.ABI_VERSION == 40


def test_new_prototypes_name_no_leading_dimension():
    import test_placement_coverage as PC
    protos = R.prototypes()
    for name in NEW:
        assert not [p for p in protos[name] if PC.NAMED.fullmatch(p)], name


def test_existing_prototypes_did_not_change():
    protos = R.prototypes()
    assert protos['spt_lookup_forward'] == ['query', 'key', 'out', 'batch_size', 'seq_length', 'n_subspaces',
                                            'sparsity', 'stream']
    assert protos['spt_attention_mfma_forward'][-4:] == ['clamp', 'heads', 'y_transposed', 'stream']
    assert protos['spt_attention_mfma_backward'][-4:] == ['clamp', 'heads', 'transposed', 'stream']
    assert 'kv_heads' not in protos['spt_attention_mfma_forward_bf16'] + protos['spt_attention_mfma_backward_bf16']


def _pointer_rows():
    from naive_gpt import ext
    protos = R.prototypes()
    return [(entry, name) for entry in NEW
            for name, ctype in zip(protos[entry], ext._PROTOTYPES[entry][0])
            if ctype is ctypes.c_void_p and name not in OPTIONAL]


@R.no_gpu
@pytest.mark.parametrize('entry,pointer', _pointer_rows())
def test_null_pointer_is_einval(lib, entry, pointer):
    assert _call(lib, entry, **{pointer: None}) == SPT_EINVAL


HEAD_COUNTS = [
    ('kv_heads == 0', dict(kv_heads=0)),
    ('kv_heads < 0', dict(kv_heads=-2)),
    ('heads == 0 (the [B, S, E] layout has no groups)', dict(heads=0)),
    ('heads < 0', dict(heads=-6)),
    ('heads % kv_heads != 0', dict(kv_heads=4)),
    ('kv_heads > heads', dict(kv_heads=12)),
    ('batch_size % heads != 0', dict(batch_size=13)),
]
# (spt_head_group_sum takes rows, not slices: no batch_size to get wrong)
HEAD_ROWS = [pytest.param(entry, what, changes, id='{}-{}'.format(entry, what.split(' (')[0]))
             for entry in NEW for what, changes in HEAD_COUNTS if set(changes) <= set(BASE[entry])]


@R.no_gpu
@pytest.mark.parametrize('entry,what,changes', HEAD_ROWS)
def test_head_counts_are_refused_with_eshape(lib, entry, what, changes):
    assert _call(lib, entry, **changes) == SPT_ESHAPE, what


@R.no_gpu
@pytest.mark.parametrize('what,changes', [('rows == 0', dict(rows=0)), ('d_head % 4 != 0', dict(d_head=66))])
def test_group_sum_shapes_are_refused_with_eshape(lib, what, changes):
    assert _call(lib, 'spt_head_group_sum', **changes) == SPT_ESHAPE, what


@R.no_gpu
@pytest.mark.parametrize('entry', NEW)
@pytest.mark.parametrize('kv_heads', [2, 6, 1])
def test_valid_head_counts_pass_validation(lib, entry, kv_heads):
    """Grouped (2 of 6), kv_heads == heads and MQA get past every check: what comes back is the
    launch's own "no device" error, a positive code, never a refusal."""
    assert _call(lib, entry, kv_heads=kv_heads) > 0


@R.no_gpu
def test_null_checks_come_before_shape_checks(lib):
    for entry in NEW:
        pointer = next(p for e, p in _pointer_rows() if e == entry)
        assert _call(lib, entry, kv_heads=0, **{pointer: None}) == SPT_EINVAL, entry

