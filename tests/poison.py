"""Poisoned allocations: make a result that depends on what a buffer held before the call visible.

`poisoned(pattern)` patches `torch.empty`, `torch.empty_like` and `torch.Tensor.new_empty` so that
every CUDA tensor they create is filled first.  `naive_gpt.ext` and the layers look these functions
up on `torch` at call time, so every wrapper's outputs, scratch and workspaces are reached.

  pattern | fp32 / bf16 | int32 / int64 / bool | uint8 workspaces
  zero    | 0           | 0                   | all bytes 0
  nan     | quiet NaN   | 1                   | each 32-bit word 1
  big     | -1.5e38     | 1                   | each word 0x7FC00000 (a NaN float) if float-only, else 1

Integers are never poisoned with large or negative values: an unwritten cursor, counter or index
poisoned that way would become an out-of-range address.  With 1, a missing zeroing shows up as a
shifted or duplicated entry instead.
"""
import collections
import contextlib
import sys

import torch

PATTERNS = ('zero', 'nan', 'big')

# The uint8 workspaces of naive_gpt/ext.py, by the wrapper that allocates them, classified from
# the kernel that uses them.  FLOAT_ONLY: only float (or double) partials, images or products live
# there, so a NaN word is a fair poison.  INDEXED: indices, counters or tile headers live there.
FLOAT_ONLY = {
    'cdist_backward_cuda': 'cdist.hip:247 per-block fp32 partials of grad_table',
    'spmm_transposed': 'spmm.hip:881-882 fp32 per-chunk outputs or permuted values',
    'grouped_gemm_wgrad': 'grouped_wgrad.hip: spt_grouped_gemm_wgrad_workspace_bytes fp32 per-chunk partials of dW and dbias (bf16: the same)',
    'split_bf16': 'grouped_gemm.hip: split_bf16_kernel stores hi / lo bf16 pairs only',
    'lora_down': 'lora_side.hip:145 the by-product split image: 128-byte hi / lo bf16 blocks',
    'lora_down_tables': 'lora_side.hip:145 (via :340) the by-product split image',
    'lora_down_grouped': 'lora_side.hip:145 (via :349) the by-product split image',
    'tall_tn': 'lora_side.hip:596 fp32 per-chunk partials',
    'tall_tn_batch': 'lora_side.hip:596 fp32 per-chunk partials, one set per pair',
    'tall_tn_bf16': 'lora_side.hip:663 fp32 per-chunk partials',
    'embedding_rows_backward': 'routing.hip:361 fp64 per-position partials',
}
INDEXED = {
    'attention_mfma_prepare': 'attention_tiles.hip: spt_attention_mfma_prepare tile header, masks and cell counts',
    'csr_transpose': 'spmm.hip:894 the transposed CSR: row pointers and column ids',
    'spmm_forward_cuda': 'spmm.hip:945 a csr_transpose structure in front of the products',
    'grouped_gemm_fused': 'grouped_gemm.hip: launch_grouped ReLU-fix queue counters and entries',
}

_NAN_WORD = 0x7FC00000


class Poison:
    """What one `poisoned` block did: CUDA buffers filled, by allocating function."""

    def __init__(self, pattern):
        self.pattern = pattern
        self.count = 0
        self.sites = collections.Counter()
        self.unclassified = set()


def _fill_words(t: torch.Tensor, word: int):
    flat = t.view(-1)
    n4 = flat.numel() // 4
    if n4:
        flat[:4 * n4].view(torch.int32).fill_(word)
    for i in range(4 * n4, flat.numel()):          # a ragged tail: the word's low bytes
        flat[i] = (word >> (8 * (i - 4 * n4))) & 0xFF


def _fill(t: torch.Tensor, state: Poison, caller: str):
    if not t.is_cuda or t.numel() == 0:
        return t
    state.count += 1
    state.sites[caller] += 1
    p = state.pattern
    with torch.no_grad():
        if p == 'zero':
            t.zero_()
        elif t.dtype == torch.uint8:
            if caller not in FLOAT_ONLY and caller not in INDEXED:
                state.unclassified.add(caller)
            _fill_words(t, _NAN_WORD if p == 'big' and caller in FLOAT_ONLY else 1)
        elif t.is_floating_point():
            t.fill_(float('nan') if p == 'nan' else -1.5e38)
        else:
            t.fill_(1)
    return t


@contextlib.contextmanager
def poisoned(pattern: str):
    assert pattern in PATTERNS, pattern
    state = Poison(pattern)
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def caller():
        return sys._getframe(2).f_code.co_name

    def p_empty(*args, **kwargs):
        return _fill(empty(*args, **kwargs), state, caller())

    def p_empty_like(*args, **kwargs):
        return _fill(empty_like(*args, **kwargs), state, caller())

    def p_new_empty(self, *args, **kwargs):
        return _fill(new_empty(self, *args, **kwargs), state, caller())

    torch.empty, torch.empty_like, torch.Tensor.new_empty = p_empty, p_empty_like, p_new_empty
    try:
        yield state
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal shapes, dtypes and bytes (NaNs compare too)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.detach().reshape(-1).contiguous().view(torch.uint8),
                       b.detach().reshape(-1).contiguous().view(torch.uint8))


def fresh_caches(*indices):
    """Empty every cache that could carry a result from one run into the next: every registered memo
    of the package (`ext.clear_memos`: split images, weight images and norms, the csr_transpose memo,
    the adapters' shared down products, and whatever registers later), the norm output last
    recomputed, and the attention layers' indptr cache.  (`indices`: what callers hand on as `*memo`;
    the transposed memo no longer needs them to be found.)"""
    from naive_gpt import ext
    from naive_gpt.layers.sparse.attention import _SparseCore
    from naive_gpt.layers.tuning import recompute
    ext.clear_memos()
    recompute.release()
    _SparseCore._indptr_cache.clear()
