"""CPU tier: the bf16 LoRA routed-FFN entries (spt_grouped_gemm_bf16_ext, spt_lora_down_bf16 and its grouped
form, spt_tall_tn_bf16 and its workspace size, spt_swiglu_backward_dots_bf16) are declared, exported and
bound, additive under ABI 40, validate their arguments on the host before any launch; and the layers' opt-in
gate (grouped.LORA_BF16, grouped.lora_bf16_usable) decides as documented."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'spt_hip.h')
NAMES = ('spt_grouped_gemm_bf16_ext', 'spt_lora_down_bf16', 'spt_lora_down_grouped_bf16', 'spt_tall_tn_bf16',
         'spt_tall_tn_bf16_workspace_bytes', 'spt_swiglu_backward_dots_bf16')
FAKE = 1 << 20      # a 16-byte aligned address that is never dereferenced: the checks come first


def _c_args(text, name):
    """the parameter count of a prototype in the header"""
    m = re.search(r'\b{}\s*\((.*?)\);'.format(name), text, flags=re.S)
    return len([p for p in m.group(1).split(',') if p.strip()])


def test_header_library_and_binding_agree_on_the_new_entries():
    from naive_gpt import ext
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    lib = ext.load_library()
    for name in NAMES:
        assert re.search(r'\b{}\s*\('.format(name), text), name
        assert name in ext._PROTOTYPES, name
        assert hasattr(lib, name), name
        assert _c_args(text, name) == len(ext._PROTOTYPES[name][0]), name
    assert 'typedef struct SptGroupedGemmBf16Ext' in text
    assert int(re.search(r'#define SPT_ABI_VERSION (\d+)', open(HEADER).read()).group(1)) == 40
    assert lib.spt_abi_version() == ext.ABI_VERSION == 40
    # the existing bf16 entries keep their prototypes
    assert ext._PROTOTYPES['spt_grouped_gemm_bf16'][0] == [ctypes.c_void_p] * 2
    assert len(ext._PROTOTYPES['spt_swiglu_backward_bf16'][0]) == 7
    # the same workspace as the fp32 tall_tn at the padded column count
    f, f32 = lib.spt_tall_tn_bf16_workspace_bytes, lib.spt_tall_tn_workspace_bytes
    assert f(0, 1, 64, 16) == 0 and f(100, 1, 64, 52) == 0
    for rows, G, width, n, npad in ((1000, 1, 1024, 16, 16), (5000, 8, 512, 8, 16), (300, 4, 64, 32, 32),
                                   (77, 1, 2, 4, 4), (9000, 2, 256, 44, 48)):
        assert f(rows, G, width, n) == f32(rows, G, width, npad)


def test_ext_descriptor_layout_matches_the_header():
    from naive_gpt import ext
    body = re.search(r'typedef struct SptGroupedGemmBf16Ext \{(.*?)\} SptGroupedGemmBf16Ext;',
                     open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'(\w+)\s*[,;]', body)
    assert fields == [f[0] for f in ext._GroupedExtBf16._fields_]
    assert ctypes.sizeof(ext._GroupedExtBf16) == 48


def _desc(**over):
    from naive_gpt import ext
    kw = dict(a=FAKE, gather=None, w=FAKE, bias=None, rowscale=None, offsets=FAKE, out=FAKE, n_rows=256,
              k=256, n=128, n_groups=4, lda=256, w_group_stride=128 * 256, w_ldn=256, w_ldk=1, ldo=0,
              epilogue=ext.EPI_PLAIN, activation=ext.ACT_RELU, accumulate=0, out2=None, h_in=None, s_in=None,
              pdot_main=None, pdot_act=None, pdot_ld=0)
    kw.update(over)
    return ext._GroupedDescBf16(**kw)


def _ext(**over):
    from naive_gpt import ext
    kw = dict(a2=FAKE, gather2=None, b2=FAKE, lda2=16, r=16, b2_group_stride=128 * 16, b2_ldn=16)
    kw.update(over)
    return ext._GroupedExtBf16(**kw)


def test_grouped_gemm_bf16_ext_validates_before_launch():
    from naive_gpt import ext
    lib = ext.load_library()

    def call(desc=None, **over):
        return lib.spt_grouped_gemm_bf16_ext(ctypes.byref(desc or _desc()), ctypes.byref(_ext(**over)), None)

    assert lib.spt_grouped_gemm_bf16_ext(ctypes.byref(_desc()), None, None) == -1
    assert lib.spt_grouped_gemm_bf16_ext(None, ctypes.byref(_ext()), None) == -1
    # the main operands are checked as spt_grouped_gemm_bf16 checks them
    assert call(_desc(a=None)) == -1 and call(_desc(k=224, lda=224, w_ldn=224, w_group_stride=128 * 224)) == -2
    assert call(_desc(epilogue=ext.EPI_ACT, accumulate=1)) == -3
    for name in ('a2', 'b2'):
        assert call(**{name: None}) == -1, name
    assert call(r=0) == -1 and call(lda2=12) == -1 and call(b2_ldn=12) == -1 and call(b2_group_stride=-4) == -1
    assert call(r=6, lda2=8, b2_ldn=8) == -3                     # r % 4
    assert call(r=36, lda2=36, b2_ldn=36) == -3                  # r <= 32
    assert call(lda2=18) == -2 and call(b2_ldn=18) == -2 and call(b2_group_stride=128 * 16 + 2) == -2
    assert call(a2=FAKE + 8) == -2                               # 16-byte a2 rows
    assert call(b2=FAKE + 4) == -2                               # 8-byte b2
    # the dX orientation takes the extension too (n-contiguous weight, k-contiguous b2)
    dx = _desc(w_ldn=1, w_ldk=256, n=256, k=128, lda=128, w_group_stride=128)
    assert call(dx, r=36, lda2=36, b2_ldn=36) == -3 and call(dx, b2=FAKE + 2) == -2


def test_lora_down_bf16_validates_before_launch():
    from naive_gpt import ext
    lib = ext.load_library()
    args = dict(x=FAKE, ldx=256, rows=100, k=256, l=FAKE, n=16, u=FAKE, ldu=0, block_major=0, stream=None)

    def call(**over):
        return lib.spt_lora_down_bf16(*dict(args, **over).values())

    for name in ('x', 'l', 'u'):
        assert call(**{name: None}) == -1, name
    assert call(rows=0) == -1 and call(k=0) == -1 and call(n=0) == -1 and call(ldx=128) == -1
    assert call(ldu=8) == -1
    assert call(n=18) == -3 and call(n=68) == -3 and call(n=8, block_major=1) == -3
    assert call(k=224, ldx=224) == -2 and call(ldx=260) == -2
    assert call(x=FAKE + 8) == -2 and call(l=FAKE + 4) == -2
    gargs = dict(x=FAKE, ldx=256, rows=100, k=256, l=FAKE, l_group_stride=256 * 16, n=16, offsets=FAKE,
                 n_groups=4, u=FAKE, ldu=0, stream=None)

    def gcall(**over):
        return lib.spt_lora_down_grouped_bf16(*dict(gargs, **over).values())

    assert gcall(offsets=None) == -1 and gcall(n_groups=0) == -1
    assert gcall(l_group_stride=256 * 8) == -1                   # tables overlap
    assert gcall(n_groups=65) == -3
    assert gcall(l_group_stride=256 * 16 + 2) == -2


def test_tall_tn_bf16_validates_before_launch():
    from naive_gpt import ext
    lib = ext.load_library()
    args = dict(wide=FAKE, ldw=128, narrow=FAKE, ldn=16, gather=None, offsets=None, n_groups=1, rows=300,
                width=128, n=16, out=FAKE, workspace=FAKE, stream=None)

    def call(**over):
        return lib.spt_tall_tn_bf16(*dict(args, **over).values())

    for name in ('wide', 'narrow', 'out', 'workspace'):
        assert call(**{name: None}) == -1, name
    assert call(rows=0) == -1 and call(ldw=64) == -1 and call(ldn=8) == -1
    assert call(n_groups=2) == -1                                # groups need offsets
    assert call(n=6, ldn=8) == -3 and call(n=52, ldn=52) == -3
    assert call(n_groups=65, offsets=FAKE) == -3
    assert call(width=127, ldw=128) == -2 and call(ldw=129) == -2 and call(ldn=18, n=16) == -2
    assert call(wide=FAKE + 2) == -2 and call(narrow=FAKE + 8) == -2 and call(out=FAKE + 1) == -2


def test_swiglu_backward_dots_bf16_validates_before_launch():
    from naive_gpt import ext
    lib = ext.load_library()
    f = lib.spt_swiglu_backward_dots_bf16
    assert f(FAKE, FAKE, FAKE, FAKE, FAKE, None, 4, 64, None) == -1
    assert f(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, 64, None) == -1
    assert f(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 62, None) == -2
    assert f(FAKE, FAKE + 4, FAKE, FAKE, FAKE, FAKE, 4, 64, None) == -2
    assert f(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE + 2, 4, 64, None) == -2


def test_bindings_refuse_dtype_mixes():
    import torch
    from naive_gpt import ext
    x = torch.zeros([64, 64], dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ext.lora_down_bf16(x.float(), torch.zeros([64, 16], dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        ext.tall_tn_bf16(x, torch.zeros([64, 16], dtype=torch.bfloat16))      # narrow stays fp32
    with pytest.raises(RuntimeError):
        ext.grouped_gemm_bf16_ext(x, x, torch.zeros([2], dtype=torch.int32), 1, 64, 64, 0, 64, 1,
                                  a2=torch.zeros([64, 16], dtype=torch.bfloat16),      # a2 stays fp32
                                  b2=torch.zeros([64, 16], dtype=torch.bfloat16), b2_group_stride=0)
    assert not ext.lora_down_bf16_supported(x, torch.zeros([64, 16]))
    assert not ext.tall_tn_bf16_supported(x.float(), torch.zeros([64, 16]))


class _Cuda(__import__('torch').Tensor):       # a CPU tensor that passes the is_cuda test of the gates
    @property
    def is_cuda(self):
        return True


def test_lora_bf16_gate_decisions(monkeypatch):
    import torch
    from naive_gpt.layers.sparse import grouped

    def t(*shape, dtype=torch.bfloat16):
        return torch.zeros(shape, dtype=dtype).as_subclass(_Cuda)

    x, w = t(8, 128), t(256, 128)
    tables = (t(128, 16), t(256, 16))
    ok = dict(rank=16, plain_router=True, d=128, bs=128, frozen=(w, None), trained=tables)

    def gate(**over):
        kw = dict(ok, **over)
        return grouped.lora_bf16_unusable(kw.pop('x', x), **kw)

    monkeypatch.setattr(grouped, 'LORA_BF16', False)
    assert 'SPT_ROUTED_LORA_BF16' in gate()
    assert not grouped.lora_bf16_usable(x, **ok)
    monkeypatch.setattr(grouped, 'LORA_BF16', True)
    assert gate() is None and grouped.lora_bf16_usable(x, **ok)
    assert 'bf16 CUDA activations' in gate(x=t(8, 128, dtype=torch.float32))
    assert 'bf16 CUDA activations' in gate(x=torch.zeros([8, 128], dtype=torch.bfloat16))
    assert 'frozen' in gate(frozen=(t(256, 128, dtype=torch.float32),))
    assert 'frozen' in gate(frozen=(t(256, 128).requires_grad_(True),))
    assert 'frozen' in gate(frozen=(t(128, 256).t(),))                            # not contiguous
    assert 'LoRA table' in gate(trained=(t(128, 16, dtype=torch.float32),))
    assert 'multiples of 64' in gate(d=96) and 'multiples of 64' in gate(bs=160)
    assert 'rank' in gate(rank=6) and 'rank' in gate(rank=64)
    assert 'router' in gate(plain_router=False)


def test_lora_layers_route_by_the_flag(monkeypatch):
    """with the flag on, a bf16 layer asks the bf16 gate and names its reason when it keeps the loop; with
    it off, the loop's note is today's"""
    import torch
    from torch import nn
    from naive_gpt import ext
    from naive_gpt.layers.sparse import grouped
    from naive_gpt.layers.tuning import lora_ffn
    torch.manual_seed(0)
    opt = lora_ffn.LoRARoutedFFN(d_lora=16, block_size=64, d_model=64, d_feedforward=256,
                                 activation=nn.ReLU()).bfloat16()
    llama = lora_ffn.LoRARoutedLLaMaFFN(d_lora=16, block_size=64, d_model=64, d_feedforward=256,
                                        activation=nn.SiLU()).bfloat16()
    for m in (opt, llama):
        for name, p in m.named_parameters():
            p.requires_grad_('lora' in name or 'router' in name)
    x = torch.randn([2, 8, 64]).bfloat16()
    xc = x.view(-1, 64).as_subclass(_Cuda)
    monkeypatch.setattr(grouped, 'LORA_BF16', True)
    # (the parameters live on the CPU here: the gate names them)
    assert 'CUDA weights' in opt._bf16_unusable(xc) and 'CUDA weights' in llama._bf16_unusable(xc)
    assert 'activation' in lora_ffn.LoRARoutedFFN(16, 64, 64, 256, nn.Tanh()).bfloat16()._bf16_unusable(xc)
    for m in (opt, llama):
        ext.reset_paths()
        y_on = m(x)                                              # CPU: the loop, with the bf16 reason
        assert ext.paths_taken('routed_ffn') == {('routed_ffn', 'torch_loop'): 1}
        monkeypatch.setattr(grouped, 'LORA_BF16', False)
        ext.reset_paths()
        y_off = m(x)
        assert ext.paths_taken('routed_ffn') == {('routed_ffn', 'torch_loop'): 1}
        assert torch.equal(y_on, y_off)
        monkeypatch.setattr(grouped, 'LORA_BF16', True)
