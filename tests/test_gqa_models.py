"""Grouped-query attention (fewer key/value heads than query heads) from the checkpoint to the
upgraded model, without a GPU: config keys, the HuggingFace weight map, checkpoint files, the dense
model against its MHA twin, the upgraded model's parameters, tuned files, and the expanded fallback
of the sparse layers on the CPU oracle stub."""
import types

import pytest
import torch

# d_model 256, 4 query heads of d_head 64, 2 kv heads: group size 2
GQA = dict(d_model=256, n_heads=4, n_layers=2, max_length=64, vocab_size=96, d_feedforward=512, p_dropout=0.0,
           n_kv_heads=2)
MHA_KEYS = ('d_model', 'n_heads', 'n_layers', 'vocab_size', 'd_feedforward', 'max_length', 'p_dropout')


def _hf_config(**extra):
    base = dict(hidden_size=256, num_attention_heads=4, num_hidden_layers=2, vocab_size=96, intermediate_size=512,
                max_position_embeddings=64)
    base.update(extra)
    return types.SimpleNamespace(**base)


def test_config_from_hf_reads_kv_heads_and_rope_theta():
    from naive_gpt.utils import checkpoint
    plain = checkpoint.config_from_hf(_hf_config())
    assert set(plain) == set(MHA_KEYS)
    # what HuggingFace writes for an MHA LLaMA: the defaults leave no key behind
    assert checkpoint.config_from_hf(_hf_config(num_key_value_heads=4, rope_theta=10000.0)) == plain
    assert checkpoint.config_from_hf(_hf_config(num_key_value_heads=None)) == plain
    gqa = checkpoint.config_from_hf(_hf_config(num_key_value_heads=2, rope_theta=500000.0))
    assert gqa == dict(plain, n_kv_heads=2, rope_theta=500000.0)
    assert checkpoint.config_from_hf(_hf_config(num_key_value_heads=1)) == dict(plain, n_kv_heads=1)
    assert checkpoint.config_from_hf(_hf_config(rope_parameters={'rope_theta': 1e6, 'rope_type': 'default'})) \
        == dict(plain, rope_theta=1e6)


def test_build_model_shapes_and_refusals():
    from naive_gpt.utils import checkpoint
    model = checkpoint.build_model('llama', dict(GQA, rope_theta=500000.0))
    mha = model.decoders[1].mha
    assert (mha.n_heads, mha.n_kv_heads) == (4, 2)
    assert mha.linear_q.weight.shape == (256, 256) and mha.linear_o.weight.shape == (256, 256)
    assert mha.linear_k.weight.shape == (128, 256) and mha.linear_v.weight.shape == (128, 256)
    assert mha.attn_fn.rope_base == 500000.0
    default = checkpoint.build_model('llama', {k: GQA[k] for k in MHA_KEYS})
    assert default.decoders[0].mha.n_kv_heads == 4 and default.decoders[0].mha.attn_fn.rope_base == 10000.0
    assert not torch.equal(mha.attn_fn.embedding.cos_cached, default.decoders[0].mha.attn_fn.embedding.cos_cached)
    # n_kv_heads == n_heads is the model without the key
    same = checkpoint.build_model('llama', dict(GQA, n_kv_heads=4))
    assert [tuple(p.shape) for p in same.parameters()] == [tuple(p.shape) for p in default.parameters()]
    with pytest.raises(ValueError, match='n_kv_heads'):
        checkpoint.build_model('llama', dict(GQA, n_kv_heads=3))
    with pytest.raises(KeyError, match='llama'):
        checkpoint.build_model('opt', dict(GQA))


def _hf_state(config, gen):
    """A HuggingFace LLaMA state dict of random tensors for `config` (names of LlamaForCausalLM)."""
    d, dff, v = config['d_model'], config['d_feedforward'], config['vocab_size']
    d_kv = config.get('n_kv_heads', config['n_heads']) * (d // config['n_heads'])
    r = lambda *shape: 0.05 * torch.randn(list(shape), generator=gen)            # noqa: E731
    state = {'model.embed_tokens.weight': r(v, d), 'model.norm.weight': 1 + r(d), 'lm_head.weight': r(v, d)}
    for i in range(config['n_layers']):
        p = 'model.layers.{}.'.format(i)
        state.update({
            p + 'self_attn.q_proj.weight': r(d, d), p + 'self_attn.k_proj.weight': r(d_kv, d),
            p + 'self_attn.v_proj.weight': r(d_kv, d), p + 'self_attn.o_proj.weight': r(d, d),
            p + 'mlp.gate_proj.weight': r(dff, d), p + 'mlp.up_proj.weight': r(dff, d),
            p + 'mlp.down_proj.weight': r(d, dff), p + 'input_layernorm.weight': 1 + r(d),
            p + 'post_attention_layernorm.weight': 1 + r(d),
            p + 'self_attn.rotary_emb.inv_freq': r(32),
        })
    return state


def test_hf_state_loads_into_a_gqa_model():
    from naive_gpt.utils import checkpoint
    hf = _hf_state(GQA, torch.Generator().manual_seed(0))
    converted = checkpoint.llama_state_from_hf(hf)
    assert converted['decoders.1.mha.linear_k.weight'].shape == (128, 256)
    model = checkpoint.build_model('llama', GQA)
    checkpoint.load_hf_state(model, 'llama', hf)
    for i in range(2):
        for ours, theirs in (('linear_q', 'q_proj'), ('linear_k', 'k_proj'), ('linear_v', 'v_proj'), ('linear_o', 'o_proj')):
            assert torch.equal(getattr(model.decoders[i].mha, ours).weight,
                               hf['model.layers.{}.self_attn.{}.weight'.format(i, theirs)])
    # into an MHA model the same state is a shape mismatch, as before
    with pytest.raises(RuntimeError, match='size mismatch'):
        checkpoint.load_hf_state(checkpoint.build_model('llama', {k: GQA[k] for k in MHA_KEYS}), 'llama', hf)


def test_logits_match_huggingface_gqa_with_rope_theta():
    T5 = pytest.importorskip('transformers')
    from naive_gpt.utils import checkpoint
    torch.manual_seed(0)
    cfg = T5.LlamaConfig(vocab_size=96, hidden_size=64, num_hidden_layers=2, intermediate_size=176,
                         num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=64,
                         rms_norm_eps=1e-6, attention_dropout=0.0, rope_theta=500000.0)
    hf = T5.LlamaForCausalLM(cfg).eval()
    config = checkpoint.config_from_hf(cfg)
    # (transformers keeps the base in the config object or in its rope parameters, by version)
    assert config['n_kv_heads'] == 2 and config['rope_theta'] == 500000.0
    model = checkpoint.build_model('llama', config).eval()
    checkpoint.load_hf_state(model, 'llama', hf.state_dict())
    x = torch.randint(0, 96, [3, 40])
    with torch.no_grad():
        want, got = hf(x)['logits'], model(x)
    assert torch.allclose(got, want, atol=1e-5), (got - want).abs().max()


def test_checkpoint_round_trip_with_and_without_the_new_keys(tmp_path):
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    torch.manual_seed(3)
    x = torch.randint(0, GQA['vocab_size'], [2, 32])
    # an MHA config: a file with exactly today's keys
    mha_config = checkpoint.config_from_hf(_hf_config(num_key_value_heads=4, rope_theta=10000.0))
    path = str(tmp_path / 'llama-mha.ckpt')
    utils.save_checkpoint(path, mha_config, checkpoint.build_model('llama', mha_config))
    raw = torch.load(path, map_location='cpu', weights_only=True)
    assert set(raw) == {'config', 'state_dict'} and set(raw['config']) == set(MHA_KEYS)
    assert utils.model_from_checkpoint(path).decoders[0].mha.n_kv_heads == 4
    # a GQA config with its base
    config = dict(GQA, rope_theta=500000.0)
    model = checkpoint.build_model('llama', config)
    path = str(tmp_path / 'llama-gqa.ckpt')
    utils.save_checkpoint(path, config, model)
    loaded_config, state = utils.load_checkpoint(path)
    assert loaded_config == config and set(state) == set(model.state_dict())
    again = utils.model_from_checkpoint(path)
    assert again.decoders[0].mha.n_kv_heads == 2 and again.decoders[0].mha.attn_fn.rope_base == 500000.0
    with torch.no_grad():
        assert torch.equal(again(x), model(x))


def _mha_twin(gqa_model, config):
    """The MHA model that computes what `gqa_model` computes: k / v weight rows repeated per group."""
    from naive_gpt.utils import checkpoint
    twin = checkpoint.build_model('llama', {k: v for k, v in config.items() if k != 'n_kv_heads'})
    state = {k: v.clone() for k, v in gqa_model.state_dict().items()}
    g = config['n_heads'] // config['n_kv_heads']
    e = config['d_model'] // config['n_heads']
    for k in list(state):
        if k.endswith(('linear_k.weight', 'linear_v.weight')):
            w = state[k]
            state[k] = w.view(config['n_kv_heads'], e, -1).repeat_interleave(g, dim=0).reshape(-1, w.size(1))
    twin.load_state_dict(state)
    return twin


@pytest.mark.parametrize('n_kv_heads', [2, 1])
def test_dense_gqa_model_equals_the_mha_model_of_the_repeated_rows(n_kv_heads):
    """float64 on the CPU: the projections of the twin compute each kv head's rows g times, the GQA
    model once and repeats them -- the same numbers; 1e-10 relative leaves room for a library GEMM
    that blocks the two widths differently."""
    from naive_gpt.utils import checkpoint
    torch.manual_seed(5)
    config = dict(GQA, n_kv_heads=n_kv_heads, rope_theta=500000.0)
    model = checkpoint.build_model('llama', config).double().eval()
    twin = _mha_twin(model, config).double().eval()
    x = torch.randint(0, config['vocab_size'], [3, 48])
    with torch.no_grad():
        got, want = model(x), twin(x)
    assert got.dtype == torch.float64
    err = float((got - want).abs().max() / want.abs().max())
    print('dense GQA (kv {}) against its MHA twin: {:.2e} relative'.format(n_kv_heads, err))
    assert err <= 1e-10
    # and the head mapping is the one that matters: another order of the kv heads is another model
    if n_kv_heads > 1:
        wrong = _mha_twin(model, config).double().eval()
        for block in wrong.decoders:
            w = block.mha.linear_k.weight.data
            w.copy_(w.view(4, 64, -1)[[0, 2, 1, 3]].reshape_as(w))
        with torch.no_grad():
            assert float((wrong(x) - want).abs().max() / want.abs().max()) > 1e-6


def _upgraded(config):
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    torch.manual_seed(0)
    return utils.upgrade_sparse(checkpoint.build_model('llama', config), d_lora=16)


def test_upgraded_model_wraps_the_narrow_projections():
    from naive_gpt import layers
    model = _upgraded(dict(GQA, rope_theta=500000.0))
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    for i in range(GQA['n_layers']):
        mha = model.decoders[i].mha
        assert (mha.n_heads, mha.n_kv_heads) == (4, 2)
        assert isinstance(mha.attn_fn, layers.SparseRotaryAttentionV2)
        assert mha.attn_fn.rope_base == 500000.0, 'the upgrader lost the rotary base'
        for name, rows in (('linear_q', 256), ('linear_k', 128), ('linear_v', 128), ('linear_o', 256)):
            lin = getattr(mha, name)
            assert isinstance(lin, layers.LoRALinear), name
            assert lin.weight.shape == (rows, 256)
            assert lin.lora.left.weight.shape == (256, 16) and lin.lora.right.weight.shape == (rows, 16)
            prefix = 'decoders.{}.mha.{}.'.format(i, name)
            assert prefix + 'weight' in frozen
            assert {prefix + 'lora.left.weight', prefix + 'lora.right.weight'} <= trainable
    # the same names as the MHA model's: only shapes differ
    plain = _upgraded({k: GQA[k] for k in MHA_KEYS})
    assert {n for n, p in plain.named_parameters() if p.requires_grad} == trainable
    assert {n for n, p in plain.named_parameters() if not p.requires_grad} == frozen
    # the rotary tables of the upgraded attention are those of the base model's
    base = layers.RotaryEmbedding(n_embeddings=2048, d_model=64, base=500000.0)
    assert torch.equal(model.decoders[0].mha.attn_fn.embedding.cos_cached, base.cos_cached)


def test_frozen_fp16_takes_the_narrow_weights():
    from naive_gpt.utils import adapter
    model = _upgraded(GQA)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if not p.requires_grad and p.dim() == 2:
                p.copy_(p.half().float())
    report = adapter.store_frozen_fp16(model)
    for i in range(GQA['n_layers']):
        for name in ('linear_k', 'linear_v'):
            key = 'decoders.{}.mha.{}.weight'.format(i, name)
            assert key in report['converted'], report['kept'].get(key)
            assert getattr(model.decoders[i].mha, name).weight.dtype == torch.float16


def test_tuned_file_round_trip_of_a_gqa_model(tmp_path):
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    config = dict(GQA, rope_theta=500000.0)
    torch.manual_seed(0)
    ckpt = str(tmp_path / 'llama-gqa.ckpt')
    utils.save_checkpoint(ckpt, config, checkpoint.build_model('llama', config))
    tuned = utils.upgrade_sparse(utils.model_from_checkpoint(ckpt), d_lora=16)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in tuned.named_parameters():
            if p.requires_grad:
                p.add_(0.05 * torch.randn(p.shape, generator=gen))
    small = str(tmp_path / 'llama-gqa-spt.ckpt')
    utils.save_tuned(small, tuned, config)
    raw = torch.load(small, map_location='cpu', weights_only=True)
    assert raw['config'] == config
    assert raw['state_dict']['decoders.0.mha.linear_k.lora.right.weight'].shape == (128, 16)
    loaded = utils.load_spt_model(ckpt, small, d_lora=16)
    sa, sb = loaded.state_dict(), tuned.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    # the tuner's own constructor and its save / resume carry the model too
    tuner = utils.SparseTuner.from_checkpoint(ckpt)
    try:
        assert tuner.model.decoders[0].mha.n_kv_heads == 2
        state = str(tmp_path / 'run.state')
        tuner.save(state)
        again = utils.SparseTuner.resume(ckpt, state)
        try:
            assert again.model.decoders[1].mha.linear_v.weight.shape == (128, 256)
        finally:
            again.release()
    finally:
        tuner.release()


@pytest.mark.parametrize('kind', ['vanilla', 'rotary'])
def test_sparse_layer_on_the_cpu_expands_and_says_so(kind, oracle_ext):
    """Off the matrix-core path the V2 layers repeat k and v per group in front of today's code: the
    result is the layer's on the repeated tensors, the gradients are those summed over each group,
    the PQ loss of an armed step is that of q and the UN-repeated k, and the path is noted."""
    from naive_gpt import ext, layers
    torch.manual_seed(0)
    cls = layers.SparseVanillaAttentionV2 if kind == 'vanilla' else layers.SparseRotaryAttentionV2
    attn = cls(d_head=64, d_codeword=8, n_codewords=16, p_dropout=0.0)
    N, S, H, KV, E = 2, 128, 4, 2, 64        # (lookup: Z = S / 8 a multiple of 16)
    q = torch.randn([N, S, H, E])
    k, v = torch.randn([N, S, KV, E]), torch.randn([N, S, KV, E])
    w = torch.randn([N, S, H, E])

    def run(expand_first, armed):
        qi, ki, vi = (t.clone().requires_grad_(True) for t in (q, k, v))
        ke, ve = (ki.repeat_interleave(2, dim=2), vi.repeat_interleave(2, dim=2)) if expand_first else (ki, vi)
        if armed:
            attn.arm()
        y = attn(qi, ke, ve, attn_mask=None)
        (y * w).sum().backward()
        return y.detach(), qi.grad, ki.grad, vi.grad, (attn.loss.detach().clone() if armed else None)

    ext.reset_paths(reasons=True)
    got = run(False, False)
    assert ext.paths_taken('attention').get(('attention', 'gqa_expanded')) == 1
    reasons = ext.fallback_reasons('attention', 'gqa_expanded')
    assert reasons and 'grouped key/value heads' in reasons[0], reasons
    want = run(True, False)
    for a, b, name in zip(got[:4], want[:4], ('y', 'grad_q', 'grad_k', 'grad_v')):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-6, atol=1e-6 * float(b.abs().max())), name
    # armed: the loss of q and of k as projected, not of its repeated copy
    armed = run(False, True)
    rot = attn._rotate if kind == 'rotary' else (lambda t: t)
    with torch.no_grad():
        loss = attn.quantizer.train_loss(rot(q)) + attn.quantizer.train_loss(rot(k))
    assert torch.equal(armed[4], loss)
    assert not attn.armed
