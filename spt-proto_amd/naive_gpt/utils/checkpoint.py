"""Checkpoint format of the fine-tuning recipe, and the HuggingFace -> naive_gpt weight map.

Format (reference: ``script/1-convert.py:188-195``, consumed by
``script/4-sparse-tuning-0.py:20-31``): ``torch.save({'config': {...}, 'state_dict':
{...}})`` where ``config`` holds exactly the keyword arguments of
``models.OPTModel`` / ``models.LLaMAModel`` and the model family is told from the file
name (``'opt'`` / ``'llama'`` in the path).

Loading uses ``weights_only=True``: a checkpoint is data, nothing in it is executed.

The weight map restates ``script/1-convert.py:8-130`` as two tables (HF parameter name
-> ours); it works on any state_dict with those names, e.g. a randomly initialised
``transformers.OPTForCausalLM(config)`` -- no download is involved here.
"""
import os
from typing import Dict, Tuple

import torch
from torch import nn

from naive_gpt import models

CONFIG_KEYS = ('d_model', 'n_heads', 'n_layers', 'vocab_size', 'd_feedforward',
               'max_length', 'p_dropout')
# Optional keys (LLaMA family): key -> the value that a config WITHOUT the key means.  A config
# holds one only when it differs from that value, so every file written before they existed, and
# every file of a model that does not need them, has exactly CONFIG_KEYS.
#   n_kv_heads  grouped-query attention: fewer key/value heads than query heads (None: n_heads)
#   rope_theta  the rotary embedding's base (LLaMA-3: 500000)
OPTIONAL_KEYS = {'n_kv_heads': None, 'rope_theta': 10000.0}


def model_family(path_or_name: str) -> str:
    name = os.path.basename(str(path_or_name)).lower()
    if 'opt' in name:
        return 'opt'
    if 'llama' in name:
        return 'llama'
    raise RuntimeError('cannot tell the model family (opt / llama) from ' + repr(path_or_name))


def build_model(family: str, config: dict) -> nn.Module:
    missing = [k for k in CONFIG_KEYS if k not in config]
    if missing:
        raise KeyError('checkpoint config lacks ' + ', '.join(missing))
    cls = {'opt': models.OPTModel, 'llama': models.LLaMAModel}[family]
    kwargs = {k: config[k] for k in CONFIG_KEYS}
    extra = {k: config[k] for k in OPTIONAL_KEYS if k in config}
    if extra.get('n_kv_heads') == config['n_heads']:
        del extra['n_kv_heads']
    if extra and family != 'llama':
        raise KeyError('checkpoint config keys {} belong to the llama family, not to {}'.format(
            sorted(extra), family))
    return cls(**kwargs, **extra)


def save_checkpoint(path: str, config: dict, model: nn.Module) -> None:
    torch.save({'config': dict(config), 'state_dict': model.state_dict()}, f=path)


def load_checkpoint(path: str, map_location='cpu') -> Tuple[dict, Dict[str, torch.Tensor]]:
    ckpt = torch.load(path, map_location=map_location, weights_only=True)
    if not isinstance(ckpt, dict) or 'config' not in ckpt or 'state_dict' not in ckpt:
        raise RuntimeError("not a naive_gpt checkpoint: expected {'config', 'state_dict'}")
    return ckpt['config'], ckpt['state_dict']


# ---------------------------------------------------------------------------- tuned files
# What tuning changed, and nothing else: script/8-dump-spt.py:16-35 compares a run's checkpoint with
# the base and keeps the tensors that moved or that the base does not have.  Here the model says
# which those are -- every entry of its state_dict that is not a frozen parameter (the adapter
# tables, the quantizers, the norms and biases that train, and all buffers) -- so no comparison and
# no second copy of the base is needed.  For LLaMA-7B: a few hundred MB instead of 27 GB.
TUNED_FORMAT = 1


def tuned_entries(model: nn.Module) -> Dict[str, torch.Tensor]:
    """name -> live tensor for every entry of ``model.state_dict()`` that is not a frozen parameter."""
    frozen = {name for name, p in model.named_parameters() if not p.requires_grad}
    return {k: t for k, t in model.state_dict().items() if k not in frozen}


def save_tuned(path: str, model: nn.Module, config: dict = None) -> None:
    torch.save({'config': dict(config) if config is not None else None, 'tuned': {'format': TUNED_FORMAT},
                'state_dict': {k: t.detach().cpu() for k, t in tuned_entries(model).items()}}, f=path)


def is_tuned(ckpt) -> bool:
    """A tuned file of either form: ``save_tuned``'s, or the reference's own ({'state_dict'} alone)."""
    return isinstance(ckpt, dict) and 'state_dict' in ckpt and ('tuned' in ckpt or 'config' not in ckpt)


def tuned_state(ckpt: dict) -> Dict[str, torch.Tensor]:
    if not is_tuned(ckpt):
        raise RuntimeError("not a tuned file: expected {'config', 'tuned', 'state_dict'} or {'state_dict'}")
    state = ckpt['state_dict']
    if 'tuned' in ckpt:
        if not isinstance(ckpt['tuned'], dict) or ckpt['tuned'].get('format') != TUNED_FORMAT:
            raise RuntimeError('tuned file of an unknown format: {!r}'.format(ckpt['tuned']))
        return dict(state)
    # the reference's file: keys as its LightningModule names them (script/8-dump-spt.py strips the
    # prefix with removeprefix; files written before that line carry it on every key)
    if state and all(k.startswith('model.') for k in state):
        state = {k[len('model.'):]: t for k, t in state.items()}
    return dict(state)


def load_tuned(path: str, map_location='cpu') -> Dict[str, torch.Tensor]:
    return tuned_state(torch.load(path, map_location=map_location, weights_only=True))


def load_tuned_into(model: nn.Module, state: Dict[str, torch.Tensor]) -> None:
    """Strict where a tuned file can be: no key the model does not have, none missing but frozen
    base weights."""
    own = model.state_dict()
    unexpected = sorted(k for k in state if k not in own)
    if unexpected:
        raise RuntimeError('the tuned file has keys the upgraded model does not: {}'.format(unexpected[:4]))
    lacking = sorted(k for k in tuned_entries(model) if k not in state)
    if lacking:
        raise RuntimeError('the tuned file lacks entries that are not frozen base weights: {}'.format(lacking[:4]))
    model.load_state_dict(state, strict=False)


def model_from_checkpoint(path: str, map_location='cpu') -> nn.Module:
    config, state = load_checkpoint(path, map_location=map_location)
    model = build_model(model_family(path), config)
    model.load_state_dict(state)
    return model


# --------------------------------------------------------------- HuggingFace weight maps

_OPT_LAYER = {
    'fc1': 'ffd.fc1', 'fc2': 'ffd.fc2',
    'self_attn.q_proj': 'mha.linear_q', 'self_attn.k_proj': 'mha.linear_k',
    'self_attn.v_proj': 'mha.linear_v', 'self_attn.out_proj': 'mha.linear_o',
    'self_attn_layer_norm': 'norm1', 'final_layer_norm': 'norm2',
}
_OPT_TOP = {
    'model.decoder.embed_tokens.weight': 'embedding.weight',
    'model.decoder.embed_positions.weight': 'learned_pe.weight',
    'model.decoder.final_layer_norm.weight': 'final_norm.weight',
    'model.decoder.final_layer_norm.bias': 'final_norm.bias',
    'lm_head.weight': 'lm_output.weight',
}
_LLAMA_LAYER = {
    'mlp.gate_proj': 'ffd.gate', 'mlp.up_proj': 'ffd.side', 'mlp.down_proj': 'ffd.down',
    'self_attn.q_proj': 'mha.linear_q', 'self_attn.k_proj': 'mha.linear_k',
    'self_attn.v_proj': 'mha.linear_v', 'self_attn.o_proj': 'mha.linear_o',
    'input_layernorm': 'norm1', 'post_attention_layernorm': 'norm2',
}
_LLAMA_TOP = {
    'model.embed_tokens.weight': 'embedding.weight',
    'model.norm.weight': 'final_norm.weight',
    'lm_head.weight': 'lm_output.weight',
}
_IGNORED_SUFFIXES = ('rotary_emb.inv_freq',)      # recomputed by layers.RotaryEmbedding


def _convert(hf_state: Dict[str, torch.Tensor], layer_prefix: str, layer_map: dict,
             top_map: dict) -> Dict[str, torch.Tensor]:
    out, unknown = {}, []
    for name, tensor in hf_state.items():
        if name.endswith(_IGNORED_SUFFIXES):
            continue
        if name in top_map:
            out[top_map[name]] = tensor
            continue
        if name.startswith(layer_prefix):
            index, _, rest = name[len(layer_prefix):].partition('.')
            module, _, leaf = rest.rpartition('.')
            if index.isdigit() and module in layer_map:
                out['decoders.{}.{}.{}'.format(index, layer_map[module], leaf)] = tensor
                continue
        unknown.append(name)
    if unknown:       # the reference asserts that every tensor was consumed (1-convert.py:69,129)
        raise RuntimeError('unmapped checkpoint tensors: ' + ', '.join(sorted(unknown)[:8]))
    return out


def opt_state_from_hf(hf_state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return _convert(hf_state, 'model.decoder.layers.', _OPT_LAYER, _OPT_TOP)


def llama_state_from_hf(hf_state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return _convert(hf_state, 'model.layers.', _LLAMA_LAYER, _LLAMA_TOP)


def config_from_hf(hf_config) -> dict:
    """``script/1-convert.py:146-160``."""
    d_ff = getattr(hf_config, 'ffn_dim', None) or hf_config.intermediate_size
    config = {
        'd_model': hf_config.hidden_size, 'n_heads': hf_config.num_attention_heads,
        'n_layers': hf_config.num_hidden_layers, 'vocab_size': hf_config.vocab_size,
        'd_feedforward': d_ff, 'max_length': hf_config.max_position_embeddings,
        'p_dropout': 0.0,
    }
    # grouped-query checkpoints (TinyLlama, Mistral, LLaMA-3) and a rotary base other than 10000:
    # written only when they differ from what their absence means (OPTIONAL_KEYS)
    n_kv_heads = getattr(hf_config, 'num_key_value_heads', None)
    if n_kv_heads is not None and int(n_kv_heads) != int(config['n_heads']):
        config['n_kv_heads'] = int(n_kv_heads)
    rope_theta = getattr(hf_config, 'rope_theta', None)
    if rope_theta is None:      # (newer transformers keep the base in the config's rope parameters)
        rope_theta = (getattr(hf_config, 'rope_parameters', None) or {}).get('rope_theta')
    if rope_theta is not None and float(rope_theta) != OPTIONAL_KEYS['rope_theta']:
        config['rope_theta'] = float(rope_theta)
    return config


def load_hf_state(model: nn.Module, family: str, hf_state: Dict[str, torch.Tensor]) -> None:
    """Copy a HuggingFace OPT / LLaMA state_dict into ``model``; buffers that HF does not
    store (``attn_mask``, rotary caches) keep their constructed values."""
    convert = {'opt': opt_state_from_hf, 'llama': llama_state_from_hf}[family]
    report = model.load_state_dict(convert(dict(hf_state)), strict=False)
    if report.unexpected_keys:
        raise RuntimeError('unexpected keys: ' + ', '.join(report.unexpected_keys[:8]))
    params = {n for n, _ in model.named_parameters()}
    lacking = [k for k in report.missing_keys if k in params]
    if lacking:
        raise RuntimeError('parameters without a source tensor: ' + ', '.join(lacking[:8]))
