"""CPU tier: the grouped weight-gradient entry (spt_grouped_gemm_wgrad, ABI 40) is declared, exported
and bound, validates its arguments on the host, and sizes its workspace without the bucket sizes."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'spt_hip.h')
NAMES = ('spt_grouped_gemm_wgrad', 'spt_grouped_gemm_wgrad_workspace_bytes')


def test_header_library_and_binding_agree_on_the_wgrad_entries():
    from naive_gpt import ext
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    lib = ext.load_library()
    for name in NAMES:
        assert re.search(r'\b{}\s*\('.format(name), text), name
        assert name in ext._PROTOTYPES, name
        assert hasattr(lib, name), name
    assert int(re.search(r'#define SPT_ABI_VERSION (\d+)', open(HEADER).read()).group(1)) == 40
    assert lib.spt_abi_version() == ext.ABI_VERSION == 40
    assert len(ext._PROTOTYPES['spt_grouped_gemm_wgrad'][0]) == 18


def test_wgrad_null_pointers_and_group_count_fail_without_a_device():
    from naive_gpt import ext
    lib = ext.load_library()
    fake = 1 << 20      # never dereferenced: the checks come first
    args = dict(g=fake, ldg=64, gather_g=None, a=fake, lda=64, gather_a=None, rowscale=None,
                offsets=fake, n_groups=4, n_rows=128, n=64, k=64, out=fake, group_stride=4096, ldn=64,
                dbias=None, workspace=fake, stream=None)

    def call(**over):
        kw = dict(args, **over)
        return lib.spt_grouped_gemm_wgrad(*kw.values())

    for name in ('g', 'a', 'offsets', 'out', 'workspace'):
        assert call(**{name: None}) == -1, name
    assert call(n_groups=0) == -1
    assert call(n_groups=-3) == -1
    assert call(n_rows=-1) == -1
    assert call(n=0) == -1
    assert call(ldg=32) == -1
    assert call(lda=32) == -1


def test_wgrad_workspace_bound_is_positive_and_monotone_in_rows():
    from naive_gpt import ext
    lib = ext.load_library()
    f = lib.spt_grouped_gemm_wgrad_workspace_bytes
    assert f(0, 1, 4, 4) > 0
    assert f(1, 0, 64, 64) == 0 and f(-1, 4, 64, 64) == 0
    for n_groups, n, k in ((1, 4, 4), (4, 1024, 1024), (8, 1024, 2048), (8, 2048, 1024)):
        last = 0
        for rows in list(range(0, 40000, 97)) + [1 << 20, 1 << 24, (1 << 31) - 1]:
            b = f(rows, n_groups, n, k)
            assert b >= last > 0 or (last == 0 and b > 0), (rows, n_groups, n, k)
            # at least one chunk partial per group plus the bias rows
            assert b >= n_groups * (n * k + n) * 4
            last = b


def test_wgrad_wrapper_has_no_cpu_fallback():
    import torch
    from naive_gpt import ext
    off = torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ext.grouped_gemm_wgrad(torch.zeros([2, 4]), torch.zeros([2, 4]), off, (4, 4, 16, 4, 1), 2)


def test_trainable_switch_defaults_off_and_keeps_the_loop(monkeypatch):
    """With the switch off (the default) trainable weights take the per-block loop, as before; on,
    a CPU input still falls back to the loop (the grouped path is GPU-only)."""
    import torch
    from torch import nn
    from naive_gpt import ext, layers
    from naive_gpt.layers.sparse import grouped
    assert grouped.TRAINABLE_WEIGHTS == (os.environ.get('SPT_ROUTED_TRAINABLE', '0') != '0')
    torch.manual_seed(0)
    m = layers.RoutedFFN(d_model=16, d_feedforward=64, block_size=16, activation=nn.ReLU())
    x = torch.randn([5, 16])
    for on in (False, True):
        monkeypatch.setattr(grouped, 'TRAINABLE_WEIGHTS', on)
        ext.reset_paths()
        m(x)
        assert ext.paths_taken('routed_ffn_plain') == {('routed_ffn_plain', 'torch_loop'): 1}
