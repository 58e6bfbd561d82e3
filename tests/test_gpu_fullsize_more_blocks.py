"""The four-stage-upgraded TransformerBlock at the block dimensions of the other checkpoints that the
reference's script/1-convert.py names: OPT-125M (d 768), OPT-2.7B (d 2560, 32 heads of 80), OPT-6.7B
(d 4096 with LayerNorm) and Sheared-LLaMA-2.7B (d 2560, RMS norms, 20 rotary heads of 128, SiLU-gated
d_ff 6912).  tests/test_gpu_fullsize_blocks.py covers OPT-1.3B and LLaMA-7B; this file is written the way
its test_upgraded_block_step_at_block_dims is, with that test's bounds, and its helpers are copied here.

What is new at these dimensions is the norm: d 768, 2560 and LayerNorm 4096 ran op by op before the
fused add + norm kernels took them (csrc/layernorm.hip: NV 3 and the wide-row form), so
`set(_paths('norm')) == {'kernel'}` is the assertion that fails without them.  Every other engine choice
is asserted as the existing test asserts it.
"""
import contextlib
import io

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

# every configuration gives >= 2048 rows and n * h >= 32
CONFIGS = {
    'opt125m': dict(family='opt', d=768, heads=12, d_ff=3072, N=4, S=512),
    'opt2b7': dict(family='opt', d=2560, heads=32, d_ff=10240, N=1, S=2048),
    'opt6b7': dict(family='opt', d=4096, heads=32, d_ff=16384, N=1, S=2048),
    'sheared2b7': dict(family='llama', d=2560, heads=20, d_ff=6912, N=2, S=2048),
}


def _worst(got, want):
    return float((got.detach().double() - want.detach().double()).abs().max()) \
        / max(float(want.detach().abs().max()), 1e-30)


@pytest.fixture(autouse=True)
def _fresh_counts():
    from naive_gpt import ext
    ext.reset_paths()
    ext.drop_images()
    yield
    ext.drop_images()
    torch.cuda.empty_cache()


def _paths(site):
    from naive_gpt import ext
    return {k[1]: v for k, v in ext.paths_taken(site).items()}


def _randomise_adapters(module, gen, scale=0.05):
    """`right` tables start at zero (a fresh adapter is the identity): give them values so that
    every LoRA product and every table gradient is exercised."""
    for name, p in module.named_parameters():
        if name.endswith('lora.right.weight'):
            p.data.copy_(scale * torch.randn(p.shape, generator=gen).to(p.device))


def _make_block(c):
    from naive_gpt import layers, utils
    d, heads, d_ff, S = c['d'], c['heads'], c['d_ff'], c['S']
    torch.manual_seed(0)
    if c['family'] == 'llama':
        block = layers.TransformerBlock(
            d_model=d, n_heads=heads, layernorm_fn=layers.LlamaRMSNorm(d),
            attention_fn=layers.RotaryAttention(d_head=d // heads, p_dropout=0.0, max_length=S),
            feedforward_fn=layers.LLaMaFeedforward(d_model=d, d_feedforward=d_ff, activation=nn.SiLU()),
            attention_bias=False, pre_norm=True)
    else:
        block = layers.TransformerBlock(
            d_model=d, n_heads=heads, layernorm_fn=nn.LayerNorm(d),
            attention_fn=layers.VanillaAttention(d_head=d // heads, p_dropout=0.0),
            feedforward_fn=layers.Feedforward(d_model=d, d_feedforward=d_ff, activation=nn.ReLU(),
                                              p_dropout=0.0),
            attention_bias=True, pre_norm=True)
    with contextlib.redirect_stdout(io.StringIO()):
        for stage in ['lora', 'ffn', 'mha_v1', 'mha_v2']:         # script/0-profile.py:183-189
            block = utils.ModuleUpgrader(utils.SparseLoRAHandler(d_lora=16, stage=stage)).visit(block)
    return block.cuda()


@pytest.mark.parametrize('name', list(CONFIGS))
def test_upgraded_block_step_at_more_block_dims(name):
    """One four-stage-upgraded TransformerBlock, forward + backward with the PQ loss armed: every engine
    choice asserted; two runs bit-identical in the output; finite everywhere; the directional derivative
    along the last adapter table (in which the block is exactly linear) equals the finite difference."""
    from naive_gpt import ext
    c = CONFIGS[name]
    assert c['N'] * c['S'] >= 2048 and c['N'] * c['heads'] >= 32
    block = _make_block(c)
    gen = torch.Generator().manual_seed(3)
    _randomise_adapters(block, gen)
    d = c['d']
    x = torch.randn([c['N'], c['S'], d], generator=gen).cuda()
    w = torch.randn([c['N'], c['S'], d], generator=gen).cuda()

    def run(arm):
        block.zero_grad()
        if arm:
            block.mha.attn_fn.arm()
        xi = x.clone().requires_grad_(True)
        y = block(xi)
        loss = (y * w).sum()
        if arm:
            loss = loss + 1e-2 * block.mha.attn_fn.loss
        loss.backward()
        return y.detach(), xi.grad, {n: p.grad.clone() for n, p in block.named_parameters()
                                     if p.grad is not None}

    ext.reset_paths()
    y1, gx1, g1 = run(True)
    print('[more blocks] {}: {}'.format(name, {k: v for k, v in sorted(ext.paths_taken().items())}))
    assert set(_paths('norm')) == {'kernel'}, _paths('norm')      # fails without the kernels at these widths
    assert _paths('qkv_projection') == {'joint': 1}
    assert _paths('attention') == {'mfma': 1}
    assert _paths('lora_linear') == {'mfma': 1} and _paths('lora_linear_backward') == {'mfma': 1}   # linear_o
    assert _paths('routed_ffn') == {'fused': 1} and _paths('route_topk') == {'kernel': 1}
    assert 'library' not in _paths('lora_down'), _paths('lora_down')
    assert set(_paths('tall_tn')) <= {'kernel', 'kernel_batch'} and set(_paths('tall_tn_blocks')) <= {'kernel', 'kernel_batch'}
    trainable = {n for n, p in block.named_parameters() if p.requires_grad}
    assert set(g1) == trainable and 'mha.attn_fn.quantizer.weight' in g1
    for t in [y1, gx1] + list(g1.values()):
        assert torch.isfinite(t).all()
    y2, gx2, g2 = run(True)
    assert torch.equal(y1, y2)
    assert _worst(gx2, gx1) <= 1e-5
    for n in g1:
        assert _worst(g2[n], g1[n]) <= 1e-4, n
    # exact linear direction: the FFN's last `right` table
    last = block.ffd.fc2 if c['family'] == 'opt' else block.ffd.down
    table = last.lora.right.weight
    direction = torch.randn(table.shape, generator=gen).cuda()
    y0, _, g0 = run(False)
    with torch.no_grad():
        table.add_(direction)
    ya, _, _ = run(False)
    with torch.no_grad():
        table.sub_(direction)
    fd = ((ya - y0).double() * w.double()).sum()
    an = (g0['ffd.{}.lora.right.weight'.format('fc2' if c['family'] == 'opt' else 'down')].double()
          * direction.double()).sum()
    assert abs(fd - an) <= 2e-3 * abs(an) + 1e-2, (float(fd), float(an))
