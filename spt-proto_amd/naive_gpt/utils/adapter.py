"""Module upgrader (reference: ``naive_gpt/utils/adapter.py``).

``ModuleUpgrader(handler).visit(root)`` walks ``root.named_modules()``, asks the
handler's ``on<ClassName>`` method (or ``default``) for a replacement of each module
and swaps the replacements in afterwards.  ``SparseLoRAHandler`` stages the SPT
conversion: ``'lora'`` (every Linear/Embedding -> LoRA), ``'ffn'`` (Feedforward ->
LoRA routed FFN with 4 blocks), ``'mha_v1'`` (attention -> dense attention + PQ
training loss, d_codeword 8, 16 codewords, d_head/8 subspaces), ``'mha_v2'``
(-> PQ sparse attention, codebook carried over).  These constants fix every
hyper-parameter of the hot path.
"""
import torch
from torch import nn

from naive_gpt import layers

D_CODEWORD = 8       # reference: adapter.py:97,115
N_CODEWORDS = 16
FFN_BLOCKS = 4       # block_size = d_ff // 4, reference: adapter.py:163,178


def _log(tag: str, name: str, child: nn.Module, new: nn.Module = None):
    if new is None:
        print(tag, name, type(child).__name__)
    else:
        print(tag, name, type(child).__name__, '->', type(new).__name__)


class LoRAHandler:
    def __init__(self, d_lora: int):
        self.d_lora = d_lora

    def default(self, name: str, child: nn.Module):
        _log('[SKIP]', name, child)

    def onLinear(self, name: str, child: nn.Linear):
        assert isinstance(child, nn.Linear)
        new_model = layers.LoRALinear.from_pretrained(d_lora=self.d_lora, source=child)
        _log('[UPGRADE]', name, child, new_model)
        return new_model

    def onEmbedding(self, name: str, child: nn.Embedding):
        assert isinstance(child, nn.Embedding)
        new_model = layers.LoRAEmbedding.from_pretrained(d_lora=self.d_lora, source=child)
        _log('[UPGRADE]', name, child, new_model)
        return new_model


class SparseLoRAHandler(LoRAHandler):
    STAGES = ('lora', 'ffn', 'mha_v1', 'mha_v2')

    def __init__(self, d_lora: int, stage: str):
        super().__init__(d_lora=d_lora)
        assert stage in self.STAGES
        self.stage = stage

    def _inactive(self, stage: str, name: str, child: nn.Module) -> bool:
        if self.stage != stage:
            _log('[SKIP]', name, child)
            return True
        return False

    def onLinear(self, name: str, child: nn.Linear):
        assert isinstance(child, nn.Linear)
        if self._inactive('lora', name, child):
            return None
        return LoRAHandler.onLinear(self, name=name, child=child)

    def onEmbedding(self, name: str, child: nn.Embedding):
        assert isinstance(child, nn.Embedding)
        if self._inactive('lora', name, child):
            return None
        return LoRAHandler.onEmbedding(self, name=name, child=child)

    def _to_v1(self, cls, name: str, child: nn.Module):
        # (a rotary attention keeps its base: LLaMA-3's rope_theta is not the default)
        extra = {'rope_base': child.rope_base} if hasattr(child, 'rope_base') else {}
        new_model = cls(d_head=child.d_head, p_dropout=child.p_dropout,
                        d_codeword=D_CODEWORD, n_codewords=N_CODEWORDS,
                        n_subspaces=child.d_head // D_CODEWORD, **extra)
        _log('[UPGRADE]', name, child, new_model)
        return new_model

    def onVanillaAttention(self, name: str, child: layers.VanillaAttention):
        if self._inactive('mha_v1', name, child):
            return None
        assert isinstance(child, layers.VanillaAttention)
        return self._to_v1(layers.SparseVanillaAttentionV1, name, child)

    def onRotaryAttention(self, name: str, child: layers.RotaryAttention):
        if self._inactive('mha_v1', name, child):
            return None
        assert isinstance(child, layers.RotaryAttention)
        return self._to_v1(layers.SparseRotaryAttentionV1, name, child)

    def _to_v2(self, cls, name: str, child: nn.Module):
        new_model = cls.from_pretrained(source=child)
        _log('[UPGRADE]', name, child, new_model)
        return new_model

    def onSparseVanillaAttentionV1(self, name: str, child: layers.SparseVanillaAttentionV1):
        if self._inactive('mha_v2', name, child):
            return None
        assert isinstance(child, layers.SparseVanillaAttentionV1)
        return self._to_v2(layers.SparseVanillaAttentionV2, name, child)

    def onSparseRotaryAttentionV1(self, name: str, child: layers.SparseRotaryAttentionV1):
        if self._inactive('mha_v2', name, child):
            return None
        assert isinstance(child, layers.SparseRotaryAttentionV1)
        return self._to_v2(layers.SparseRotaryAttentionV2, name, child)

    def _to_routed(self, cls, name: str, child: nn.Module):
        new_model = cls.from_pretrained(
            d_lora=self.d_lora, block_size=child.d_feedforward // FFN_BLOCKS,
            source=child
        )
        _log('[UPGRADE]', name, child, new_model)
        return new_model

    def onFeedforward(self, name: str, child: layers.Feedforward):
        if self._inactive('ffn', name, child):
            return None
        assert isinstance(child, layers.Feedforward)
        return self._to_routed(layers.LoRARoutedFFN, name, child)

    def onLLaMaFeedforward(self, name: str, child: layers.LLaMaFeedforward):
        if self._inactive('ffn', name, child):
            return None
        assert isinstance(child, layers.LLaMaFeedforward)
        return self._to_routed(layers.LoRARoutedLLaMaFFN, name, child)


def _frozen_block_weights(model: nn.Module):
    """(name, owner module, attribute) of every frozen base weight `store_frozen_fp16` considers: the
    base `weight` of every LoRALinear of the upgraded model -- the projections of the attentions and
    the block weights of LoRARoutedFFN / LoRARoutedLLaMaFFN (their fc1 / fc2, gate / side / down are
    LoRALinears) -- except the LM head, which stays fp32 with the embeddings, norms, biases, LoRA
    tables, routers and PQ codebooks."""
    head = getattr(model, 'lm_output', None)
    for name, module in model.named_modules():
        if isinstance(module, layers.LoRALinear) and module is not head:
            yield (name + '.weight' if name else 'weight'), module


def _refuse_lossy_load(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                       error_msgs):
    """load_state_dict pre-hook of a LoRALinear whose weight `store_frozen_fp16` converted: torch copies
    an incoming tensor into the parameter's dtype, which would ROUND a fp32 tensor off the fp16 grid
    without a word -- the lossy case `store_frozen_fp16` exists to refuse.  Such a load raises."""
    t = state_dict.get(prefix + 'weight')
    if module.weight.dtype != torch.float16 or not torch.is_tensor(t) or t.dtype == torch.float16:
        return
    if not t.is_floating_point() or not torch.equal(t.detach().half().to(t.dtype), t.detach()):
        raise ValueError('load_state_dict: {}weight is stored in fp16 (store_frozen_fp16) and the incoming {} '
                         'tensor holds values that fp16 does not represent exactly; load it into a fp32-stored '
                         'model, or convert it after loading with strict=False'.format(prefix, t.dtype))


def store_frozen_fp16(model: nn.Module, strict: bool = True) -> dict:
    """Store the frozen base weights of an upgraded model in fp16, in place: half their memory, the
    same bits out of every layer.

    The matrix-core path never multiplies a weight's fp32 value but its split-bf16 image
    (hi = bf16(x), lo = bf16(x - hi)); for a value that a half represents (at most 11 significant
    bits -- what the upcast of a checkpoint published in fp16 holds) the split is exact and the image
    made from the half is byte for byte the image made from the fp32 value.  Nothing in the upgraded
    model ever writes these weights.

    A weight is converted when it does not require a gradient, is fp32, has both dimensions multiples
    of 32 (the image path then always applies) and `w.half().float()` equals `w` everywhere.  A weight
    that fails the VALUE test raises under `strict` (naming it) and stays fp32 otherwise; no value ever
    changes -- nor later: loading a state dict whose tensor for a converted weight is off the fp16 grid
    raises instead of rounding it (`_refuse_lossy_load`).  Returns {'converted': [names], 'bytes_freed': int, 'kept': {name: why}}."""
    report = {'converted': [], 'bytes_freed': 0, 'kept': {}}
    todo = []
    for name, module in _frozen_block_weights(model):
        w = module.weight
        if w.dtype == torch.float16:
            report['kept'][name] = 'stored in fp16 already'
        elif w.requires_grad:
            report['kept'][name] = 'trainable'
        elif w.dtype != torch.float32:
            report['kept'][name] = ('{}: fp16 storage serves fp32 modules only (it is exact under the fp32 '
                                    'split-bf16 arithmetic; bf16 modules round)'.format(w.dtype))
        elif w.dim() != 2 or w.size(0) % 32 != 0 or w.size(1) % 32 != 0:
            report['kept'][name] = 'shape {}: both dimensions must be multiples of 32 (image path)'.format(
                tuple(w.shape))
        else:
            with torch.no_grad():
                half = w.detach().half()
                exact = bool(torch.equal(half.float(), w.detach()))
            if exact:
                todo.append((name, module, half))
            elif strict:
                raise ValueError('store_frozen_fp16: {} holds values that fp16 does not represent exactly '
                                 '(strict=False keeps such a tensor in fp32); nothing was converted'.format(name))
            else:
                report['kept'][name] = 'holds values that fp16 does not represent exactly'
    for name, module, half in todo:            # (only now: a strict failure leaves the model as it was)
        freed = module.weight.numel() * 2
        # (`.data`: the Parameter object, its hooks and its place in the module stay; frozen, so no
        # gradient of another dtype will ever meet it)
        module.weight.data = half.contiguous()
        if not getattr(module, '_frozen_fp16_guarded', False):
            module._register_load_state_dict_pre_hook(_refuse_lossy_load, with_module=True)
            module._frozen_fp16_guarded = True
        report['converted'].append(name)
        report['bytes_freed'] += freed
    if todo and any(half.is_cuda for _, _, half in todo):
        from naive_gpt import ext
        ext.drop_images()                      # by-products keyed on the old storage
    return report


class ModuleUpgrader:
    def __init__(self, handler: object):
        if not hasattr(handler, 'default'):
            raise RuntimeError('requires default handler')
        self.handler = handler

    def visit(self, root: nn.Module) -> nn.Module:
        # 1. collect replacements; dispatch on the exact class name, so subclasses
        #    are not caught by their parents' hooks (reference: adapter.py:198-203)
        replacements = {}
        for name, child in root.named_modules():
            hook = getattr(self.handler, 'on' + type(child).__name__, None)
            if hook is None:
                hook = self.handler.default
            new_child = hook(name=name, child=child)
            if new_child is None or new_child is child:
                continue
            assert isinstance(new_child, nn.Module)
            replacements[name] = new_child
        # 2. swap them in through their parents
        for path, new_child in replacements.items():
            parent_path, _, leaf = path.rpartition('.')
            parent = root.get_submodule(parent_path) if parent_path else root
            parent.add_module(leaf, module=new_child)
        return root
