"""Every public entry of naive_gpt/ext.py that launches a kernel is called by one of the three arithmetic
tiers -- exact (test_gpu_exact_arithmetic.py), split / bf16 contract (test_gpu_arith_contract.py), fp32
contract (test_gpu_fp32_contract.py) -- or has a reason here why no floating-point bound applies to it."""
from test_exact_coverage import called_by_tiers
from test_poison_coverage import launching_entries

TIERS = ('test_gpu_exact_arithmetic.py', 'test_gpu_arith_contract.py', 'test_gpu_fp32_contract.py')

INTEGER = 'integer-only outputs'
EXEMPT = {
    'lookup_forward_cuda': INTEGER,
    'route_topk': INTEGER + ' (route_topk_coeff, the same launch with its coefficient by-product, has a case)',
    'pq_encode_heads': INTEGER,
    'cdist_encode': INTEGER,
    'image_of': 'a memo in front of split_bf16 (its case)',
    'weight_image': 'a per-parameter memo in front of split_bf16 (its case)',
    'cdist_forward_cuda': 'bit-exact against the oracle already (tests/test_gpu_kernels.py)',
}


def test_every_launching_entry_is_in_an_arithmetic_tier():
    entries = launching_entries()
    assert len(entries) > 40 and {'add_layernorm_forward', 'cross_entropy_grad_', 'pq_loss_backward_pair',
                                  'sparse_attention_backward_rows'} <= set(entries)
    covered = called_by_tiers(TIERS)
    missing = [e for e in entries if e not in covered and e not in EXEMPT]
    assert not missing, 'launching entries with neither a case in {} nor an EXEMPT reason: {}'.format(
        ' / '.join(TIERS), missing)
    stale = [e for e in EXEMPT if e not in entries or e in covered]
    assert not stale, 'EXEMPT names entries that ext.py no longer has or that have a case: {}'.format(stale)
    assert all(reason.strip() for reason in EXEMPT.values())
