"""CPU tier: the bf16 routed-FFN entries (spt_grouped_gemm_bf16, spt_grouped_gemm_wgrad_bf16 and its
workspace size, spt_rows_combine_bf16, spt_swiglu_*_bf16) are declared, exported and bound, additive
under ABI 40, and validate their arguments on the host before any launch."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'spt_hip.h')
NAMES = ('spt_grouped_gemm_bf16', 'spt_grouped_gemm_wgrad_bf16', 'spt_grouped_gemm_wgrad_bf16_workspace_bytes',
         'spt_rows_combine_bf16', 'spt_swiglu_forward_bf16', 'spt_swiglu_backward_bf16')
FAKE = 1 << 20      # a 16-byte aligned address that is never dereferenced: the checks come first


def test_header_library_and_binding_agree_on_the_bf16_entries():
    from naive_gpt import ext
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    lib = ext.load_library()
    for name in NAMES:
        assert re.search(r'\b{}\s*\('.format(name), text), name
        assert name in ext._PROTOTYPES, name
        assert hasattr(lib, name), name
    assert 'typedef struct SptGroupedGemmBf16' in text
    assert int(re.search(r'#define SPT_ABI_VERSION (\d+)', open(HEADER).read()).group(1)) == 40
    assert lib.spt_abi_version() == ext.ABI_VERSION == 40
    # same arguments as the fp32 weight-gradient entry
    assert ext._PROTOTYPES['spt_grouped_gemm_wgrad_bf16'] == ext._PROTOTYPES['spt_grouped_gemm_wgrad']


def test_descriptor_layout_matches_the_header():
    """the ctypes descriptor has the header's fields in the header's order"""
    from naive_gpt import ext
    body = re.search(r'typedef struct SptGroupedGemmBf16 \{(.*?)\} SptGroupedGemmBf16;', open(HEADER).read(),
                     flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'(\w+)\s*[,;]', body)
    assert fields == [f[0] for f in ext._GroupedDescBf16._fields_]


def _desc(**over):
    from naive_gpt import ext
    kw = dict(a=FAKE, gather=None, w=FAKE, bias=None, rowscale=None, offsets=FAKE, out=FAKE, n_rows=256,
              k=256, n=128, n_groups=4, lda=256, w_group_stride=128 * 256, w_ldn=256, w_ldk=1, ldo=0,
              epilogue=ext.EPI_PLAIN, activation=ext.ACT_RELU, accumulate=0, out2=None, h_in=None, s_in=None,
              pdot_main=None, pdot_act=None, pdot_ld=0)
    kw.update(over)
    return ext._GroupedDescBf16(**kw)


def test_grouped_gemm_bf16_validates_before_launch():
    from naive_gpt import ext
    lib = ext.load_library()

    def call(**over):
        return lib.spt_grouped_gemm_bf16(ctypes.byref(_desc(**over)), None)

    assert lib.spt_grouped_gemm_bf16(None, None) == -1
    for name in ('a', 'w', 'offsets', 'out'):
        assert call(**{name: None}) == -1, name
    for name in ('n_rows', 'k', 'n', 'n_groups'):
        assert call(**{name: 0}) == -1, name
    assert call(lda=128) == -1                                   # lda < k
    assert call(ldo=64) == -1                                    # ldo < n
    assert call(epilogue=7) == -1
    assert call(epilogue=ext.EPI_ACT, activation=9) == -3        # SPT_EUNSUP
    assert call(epilogue=ext.EPI_ACT, accumulate=1) == -3
    assert call(w_ldn=4, w_ldk=4) == -3                          # neither orientation
    # shapes and alignment: SPT_ESHAPE
    assert call(k=224, lda=224, w_ldn=224, w_group_stride=128 * 224) == -2       # k % 64
    assert call(lda=260) == -2                                   # lda % 8
    assert call(w_group_stride=128 * 256 + 4) == -2
    assert call(a=FAKE + 8) == -2 and call(w=FAKE + 2) == -2     # 16-byte rows
    assert call(out=FAKE + 2) == -2 and call(bias=FAKE + 4) == -2
    assert call(w_ldn=260) == -2                                 # k-contiguous weight rows
    # n-contiguous weights: n % 32, w_ldk % 8, w_ldk >= n
    assert call(w_ldn=1, w_ldk=256, n=112, w_group_stride=256) == -2
    assert call(w_ldn=1, w_ldk=100, n=96, w_group_stride=256) == -2
    # the derivative epilogue: saved activations, and both row-dot buffers or neither
    assert call(epilogue=ext.EPI_DACT) == -1
    assert call(epilogue=ext.EPI_DACT, activation=ext.ACT_GELU, h_in=FAKE) == -1
    assert call(epilogue=ext.EPI_DACT, s_in=FAKE, pdot_main=FAKE) == -1
    assert call(epilogue=ext.EPI_DACT, s_in=FAKE, pdot_main=FAKE, pdot_act=FAKE, pdot_ld=1) == -2


def test_wgrad_bf16_validates_before_launch():
    from naive_gpt import ext
    lib = ext.load_library()
    args = dict(g=FAKE, ldg=64, gather_g=None, a=FAKE, lda=64, gather_a=None, rowscale=None,
                offsets=FAKE, n_groups=4, n_rows=128, n=64, k=64, out=FAKE, group_stride=4096, ldn=64,
                dbias=None, workspace=FAKE, stream=None)

    def call(**over):
        return lib.spt_grouped_gemm_wgrad_bf16(*dict(args, **over).values())

    for name in ('g', 'a', 'offsets', 'out', 'workspace'):
        assert call(**{name: None}) == -1, name
    assert call(n_groups=0) == -1 and call(n_rows=-1) == -1 and call(n=0) == -1
    assert call(ldg=32) == -1 and call(lda=32) == -1
    assert call(n=62, ldg=62) == -2 and call(out=FAKE + 4) == -2 and call(dbias=FAKE + 2) == -2
    assert call(g=FAKE + 4) == -2 and call(a=FAKE + 6) == -2
    assert call(workspace=FAKE + 8) == -2                        # the fp32 partials: 16 bytes


def test_wgrad_bf16_workspace_bound():
    from naive_gpt import ext
    lib = ext.load_library()
    f, f32 = lib.spt_grouped_gemm_wgrad_bf16_workspace_bytes, lib.spt_grouped_gemm_wgrad_workspace_bytes
    assert f(1, 0, 64, 64) == 0 and f(-1, 4, 64, 64) == 0
    for n_groups, n, k in ((1, 4, 4), (4, 1024, 1024), (8, 2048, 1024)):
        last = 0
        for rows in list(range(0, 40000, 331)) + [1 << 20, (1 << 31) - 1]:
            b = f(rows, n_groups, n, k)
            assert b >= last and b >= n_groups * (n * k + n) * 4       # fp32 partials, one per group at least
            assert b == f32(rows, n_groups, n, k)
            last = b


def test_rows_combine_and_swiglu_bf16_validate_before_launch():
    from naive_gpt import ext
    lib = ext.load_library()
    assert lib.spt_rows_combine_bf16(None, FAKE, None, FAKE, 4, 2, 64, None) == -1
    assert lib.spt_rows_combine_bf16(FAKE, FAKE, None, FAKE, 0, 2, 64, None) == -1
    assert lib.spt_rows_combine_bf16(FAKE, FAKE, None, FAKE, 4, 2, 62, None) == -2
    assert lib.spt_rows_combine_bf16(FAKE + 2, FAKE, None, FAKE, 4, 2, 64, None) == -2
    assert lib.spt_swiglu_forward_bf16(None, FAKE, FAKE, 64, None) == -1
    assert lib.spt_swiglu_forward_bf16(FAKE, FAKE, FAKE, 62, None) == -2
    assert lib.spt_swiglu_backward_bf16(FAKE, FAKE, FAKE, FAKE, None, 64, None) == -1
    assert lib.spt_swiglu_backward_bf16(FAKE, FAKE, FAKE + 4, FAKE, FAKE, 64, None) == -2


def test_layer_gates_refuse_dtype_mixes():
    import torch
    from naive_gpt.layers.sparse import grouped
    x = torch.zeros([4, 64], dtype=torch.bfloat16)
    w = torch.zeros([64, 64])
    assert grouped.dtype_mix(x, w.bfloat16()) is None
    assert 'one dtype per layer' in grouped.dtype_mix(x, w)
    assert grouped.bf16_shapes(1024, 1024) and not grouped.bf16_shapes(1024, 96)


def test_lora_gate_stays_fp32_and_loop_notes_name_the_shape():
    """grouped.usable (the LoRA routed variants' gate) takes fp32 only; the plain layers' bf16 gate is
    bf16_usable, and a bf16 layer whose shapes the bf16 kernels do not take says so when it falls back"""
    import torch
    from naive_gpt.layers.sparse import feedforward, grouped

    class Cuda(torch.Tensor):          # a CPU tensor that passes the is_cuda test of the gates
        @property
        def is_cuda(self):
            return True

    x = torch.zeros([4, 96], dtype=torch.bfloat16).as_subclass(Cuda)
    w = torch.zeros([96, 96], dtype=torch.bfloat16).as_subclass(Cuda)
    assert not grouped.usable(x, w)
    assert grouped.bf16_usable(x, w) and not grouped.bf16_usable(x, w.float())
    assert feedforward._grouped_usable(x, w)
    why = feedforward._loop_why(x, False, 96, 96, w)
    assert 'multiples of 64' in why
    assert 'one dtype per layer' in feedforward._loop_why(x, False, 128, 128, w.float())
