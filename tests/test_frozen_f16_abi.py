"""Frozen base weights stored in fp16, without a GPU: the two additive C entries
(`spt_split_f16`, `spt_grouped_gemm_fused_w16`) are declared, bound and validate their arguments on the
host, and `store_frozen_fp16` converts exactly the tensors it may, changes no value and keeps the
checkpoint round trip working in both directions."""
import ctypes
import io
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'spt_hip.h')
NEW = ('spt_split_f16', 'spt_grouped_gemm_fused_w16')
CONFIG = dict(d_model=64, n_heads=2, n_layers=2, vocab_size=100, d_feedforward=256, max_length=32, p_dropout=0.0)


def test_header_and_binding_declare_both_entries_under_abi_40():
    from naive_gpt import ext
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name + ' is not declared in spt_hip.h'
        assert name in ext._PROTOTYPES, name + ' is not bound in ext._PROTOTYPES'
    assert re.search(r'spt_split_f16\s*\(\s*const void \*src_f16,\s*void \*image,\s*long long rows,\s*int cols,'
                     r'\s*long long ld,\s*void \*stream\)', text)
    assert re.search(r'spt_grouped_gemm_fused_w16\s*\(\s*const SptGroupedGemm \*\w+,\s*void \*stream\)', text)
    assert ext._PROTOTYPES['spt_split_f16'] == ext._PROTOTYPES['spt_split_bf16']
    assert ext._PROTOTYPES['spt_grouped_gemm_fused_w16'] == ext._PROTOTYPES['spt_grouped_gemm_fused']
    assert int(re.search(r'#define SPT_ABI_VERSION (\d+)', open(HEADER).read()).group(1)) == 40
    assert ext.ABI_VERSION == 40 and ext.load_library().spt_abi_version() == 40
    # the descriptor keeps its layout: the fp16 entry reads the same struct
    assert ctypes.sizeof(ext._GroupedDesc) == 280


def test_null_pointers_are_refused_before_any_launch():
    from naive_gpt import ext
    lib = ext.load_library()
    assert lib.spt_split_f16(None, None, 4, 32, 32, None) == -1
    assert lib.spt_grouped_gemm_fused_w16(None, None) == -1
    desc = ext._GroupedDesc(n_rows=128, k=32, n=32, n_groups=1, lda=32, w_ldn=32, w_ldk=1)
    assert lib.spt_grouped_gemm_fused_w16(ctypes.byref(desc), None) == -1        # every pointer NULL
    # shape preconditions of the split, also on the host: 16-byte rows of halves
    buf = (ctypes.c_char * 4096)()
    at = (ctypes.addressof(buf) + 15) & ~15
    assert lib.spt_split_f16(at, at + 1024, 4, 32, 36, None) == -2               # ld % 8 != 0
    assert lib.spt_split_f16(at + 2, at + 1024, 4, 32, 32, None) == -2           # source not 16-byte aligned
    assert lib.spt_split_f16(at, at + 1024, 4, 32, 24, None) == -1               # ld < cols
    # halves without an image: no register-operand form (SPT_EUNSUP), told before the device is asked
    desc = ext._GroupedDesc(a=at, w=at, offsets=at, out=at, n_rows=128, k=32, n=32, n_groups=1, lda=32,
                            w_ldn=32, w_ldk=1)
    assert lib.spt_grouped_gemm_fused_w16(ctypes.byref(desc), None) == -3


def _upgraded(kind='opt', grid=True):
    """A small upgraded model (the CPU stages: LoRA linears and routed FFNs), weights on the fp16 grid."""
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    torch.manual_seed(0)
    model = checkpoint.build_model(kind, dict(CONFIG))
    if grid:
        with torch.no_grad():
            for p in model.parameters():
                p.copy_(p.half().float())
    return utils.upgrade_sparse(model, d_lora=16, stages=('lora', 'ffn'))


def _frozen_weights(model):
    from naive_gpt import layers
    return {n + '.weight': m.weight for n, m in model.named_modules()
            if isinstance(m, layers.LoRALinear) and m is not model.lm_output}


@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_representable_weights_become_fp16_and_nothing_else_moves(kind):
    from naive_gpt import utils
    model = _upgraded(kind)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    trained = {n: p.requires_grad for n, p in model.named_parameters()}
    wanted = _frozen_weights(model)
    assert len(wanted) == 2 * (4 + (2 if kind == 'opt' else 3))      # q k v o + the FFN's block weights
    report = utils.store_frozen_fp16(model)
    assert sorted(report['converted']) == sorted(wanted) and report['kept'] == {}
    assert report['bytes_freed'] == sum(2 * before[n].numel() for n in wanted)
    for n, p in model.named_parameters():
        if n in wanted:
            assert p.dtype == torch.float16 and not p.requires_grad
            assert torch.equal(p.detach().float(), before[n]), n
        else:                       # biases, norms, embeddings, the LM head, LoRA tables, routers
            assert p.dtype == torch.float32 and torch.equal(p.detach(), before[n]), n
            assert p.requires_grad == trained[n], n
    assert model.lm_output.weight.dtype == torch.float32 and model.embedding.weight.dtype == torch.float32
    # a second call finds nothing to do
    again = utils.store_frozen_fp16(model)
    assert again['converted'] == [] and again['bytes_freed'] == 0 and sorted(again['kept']) == sorted(wanted)


def test_the_cpu_forward_and_backward_keep_their_bits():
    """Off the GPU a fp16-stored weight is upcast for the call (exact) and the fallback is noted."""
    from naive_gpt import ext, utils
    model = _upgraded('opt')
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith('lora.right.weight'):
                p.copy_(0.02 * torch.randn(p.shape))
    x = torch.randint(0, CONFIG['vocab_size'], [2, 16])
    want = model(x)
    want.square().sum().backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    utils.store_frozen_fp16(model)
    ext.reset_paths()
    got = model(x)
    got.square().sum().backward()
    assert torch.equal(got, want)
    for n, p in model.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, grads[n]), n
    assert ext.paths_taken('routed_ffn').get(('routed_ffn', 'f16_upcast'), 0) > 0
    # ... and so do the attention's LoRA linears (q, k, v, o of two layers), never silently
    assert ext.paths_taken('lora_linear').get(('lora_linear', 'f16_upcast'), 0) >= 8


def test_a_value_off_the_fp16_grid_raises_or_stays_fp32():
    from naive_gpt import utils
    model = _upgraded('opt')
    name = 'decoders.1.ffd.fc1.weight'
    w = model.get_parameter(name)
    with torch.no_grad():
        w[3, 5] = 1.0 + 2.0 ** -12                                  # 13 significant bits
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    with pytest.raises(ValueError, match=re.escape(name)):
        utils.store_frozen_fp16(model, strict=True)
    for n, p in model.named_parameters():                           # a strict failure converts nothing
        assert p.dtype == torch.float32 and torch.equal(p.detach(), before[n]), n
    report = utils.store_frozen_fp16(model, strict=False)
    assert name in report['kept'] and 'exactly' in report['kept'][name] and name not in report['converted']
    assert w.dtype == torch.float32 and torch.equal(w.detach(), before[name])
    assert len(report['converted']) == len(_frozen_weights(model)) - 1
    for n in report['converted']:
        assert torch.equal(model.get_parameter(n).detach().float(), before[n])


def test_a_dimension_off_the_32_grid_and_a_trainable_weight_are_kept():
    from naive_gpt import layers, utils
    torch.manual_seed(1)
    model = torch.nn.Sequential()
    model.add_module('even', layers.LoRALinear(d_lora=16, in_features=64, out_features=96))
    model.add_module('odd', layers.LoRALinear(d_lora=16, in_features=64, out_features=40))
    model.add_module('trained', layers.LoRALinear(d_lora=16, in_features=64, out_features=64))
    model.trained.weight.requires_grad = True
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.half().float())
    report = utils.store_frozen_fp16(model)
    assert report['converted'] == ['even.weight'] and report['bytes_freed'] == 96 * 64 * 2
    assert 'multiples of 32' in report['kept']['odd.weight'] and report['kept']['trained.weight'] == 'trainable'
    assert model.even.weight.dtype == torch.float16 and model.even.bias.dtype == torch.float32
    assert model.odd.weight.dtype == model.trained.weight.dtype == torch.float32
    assert model.trained.weight.requires_grad
    # bf16 activations are refused with a reason, not served from an upcast
    with pytest.raises(RuntimeError, match='fp32 modules only'):
        model.even(torch.zeros([4, 64], dtype=torch.bfloat16))


def test_checkpoint_round_trip_in_both_directions(tmp_path):
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    stored, plain = _upgraded('opt'), _upgraded('opt')
    report = utils.store_frozen_fp16(stored)
    want = {n: p.detach().clone() for n, p in plain.named_parameters()}
    # saving a converted model: half the bytes of the converted tensors, every value as it was
    path = str(tmp_path / 'opt-stored.ckpt')
    checkpoint.save_checkpoint(path, CONFIG, stored)
    _, state = checkpoint.load_checkpoint(path)
    assert all(state[n].dtype == torch.float16 for n in report['converted'])
    assert all(torch.equal(state[n].float(), want[n]) for n in want)
    # fp16 state into a fp32 model, fp32 state into a fp16 model, and each into its own kind
    for target, source in ((_upgraded('opt', grid=False), stored), (stored, plain), (plain, plain),
                           (stored, stored)):
        buf = io.BytesIO()
        torch.save(source.state_dict(), buf)
        buf.seek(0)
        dtypes = {n: p.dtype for n, p in target.named_parameters()}
        result = target.load_state_dict(torch.load(buf, weights_only=True))
        assert not result.missing_keys and not result.unexpected_keys
        for n, p in target.named_parameters():
            assert p.dtype == dtypes[n] and torch.equal(p.detach().float(), want[n]), n


def test_a_state_off_the_fp16_grid_is_not_rounded_into_a_converted_model():
    """torch's `copy_` would round such a tensor into the fp16 parameter without a word: the load raises,
    names the tensor, and the stored halves keep their values."""
    from naive_gpt import utils
    stored, plain = _upgraded('opt'), _upgraded('opt')
    utils.store_frozen_fp16(stored)
    name = 'decoders.1.ffd.fc1.weight'
    before = stored.get_parameter(name).detach().clone()
    state = plain.state_dict()
    state[name] = state[name].clone()
    state[name][3, 5] = 1.0 + 2.0 ** -12                            # 13 significant bits
    with pytest.raises(ValueError, match=re.escape(name)):
        stored.load_state_dict(state)
    assert stored.get_parameter(name).dtype == torch.float16 and torch.equal(stored.get_parameter(name), before)
    # the same state into the fp32-stored model: taken as it is
    plain.load_state_dict(state)
    assert plain.get_parameter(name)[3, 5] == 1.0 + 2.0 ** -12


def test_the_keywords_reach_the_function():
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint, tuning
    torch.manual_seed(0)
    model = checkpoint.build_model('opt', dict(CONFIG))
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.half().float())
    model = tuning.upgrade_sparse(model, d_lora=16, stages=('lora', 'ffn'), frozen_fp16=True)
    assert len(model.frozen_fp16_report['converted']) == 12
    tuner = utils.SparseTuner(_upgraded('opt'), frozen_fp16=True)
    assert len(tuner.frozen_fp16_report['converted']) == 12
    assert utils.SparseTuner(_upgraded('opt')).frozen_fp16_report is None
    assert all(p.dtype == torch.float32 for p in tuner.params)
