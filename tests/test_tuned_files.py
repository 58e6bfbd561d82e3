"""Tuned files (utils/checkpoint.py: save_tuned / load_tuned) and the evaluator's loader on them: what
tuning changed and nothing else, in this package's format or the reference's own {'state_dict'}
(script/8-dump-spt.py), on the tiny checkpoint of test_loaders.py."""
import os

import pytest
import torch


def _files(tmp_path):
    from naive_gpt import loaders, models, utils
    tok = loaders.ByteTokenizer()
    torch.manual_seed(0)
    config = dict(d_model=128, n_heads=2, n_layers=2, max_length=256, vocab_size=tok.vocab_size,
                  d_feedforward=512, p_dropout=0.0)
    ckpt = str(tmp_path / 'opt-tiny.ckpt')
    utils.save_checkpoint(ckpt, config, models.OPTModel(**config))
    tuned = utils.upgrade_sparse(utils.model_from_checkpoint(ckpt), d_lora=16)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in tuned.named_parameters():
            if p.requires_grad:                              # every trained tensor moved
                p.add_(0.05 * torch.randn(p.shape, generator=gen))
    return config, ckpt, tuned


def _same_model(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_tuned_file_round_trip_holds_no_frozen_weight_and_is_smaller(tmp_path):
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    config, ckpt, tuned = _files(tmp_path)
    full, small = str(tmp_path / 'opt-tiny-full.ckpt'), str(tmp_path / 'opt-tiny-spt.ckpt')
    utils.save_checkpoint(full, config, tuned)
    utils.save_tuned(small, tuned, config)
    raw = torch.load(small, map_location='cpu', weights_only=True)
    assert set(raw) == {'config', 'tuned', 'state_dict'} and raw['tuned'] == {'format': 1} and raw['config'] == config
    frozen = {n for n, p in tuned.named_parameters() if not p.requires_grad}
    assert frozen and not frozen & set(raw['state_dict'])
    assert set(raw['state_dict']) == set(tuned.state_dict()) - frozen
    assert any('lora' in k for k in raw['state_dict'])
    assert os.path.getsize(small) < os.path.getsize(full)
    assert os.path.getsize(small) < os.path.getsize(ckpt), 'adapters larger than the base they adapt'
    assert set(checkpoint.load_tuned(small)) == set(raw['state_dict'])
    _same_model(utils.load_spt_model(ckpt, small, d_lora=16), tuned)
    # today's second file, the whole upgraded model, loads as before
    _same_model(utils.load_spt_model(ckpt, full, d_lora=16), tuned)
    # without a config
    utils.save_tuned(small, tuned)
    assert torch.load(small, map_location='cpu', weights_only=True)['config'] is None
    _same_model(utils.load_spt_model(ckpt, small, d_lora=16), tuned)


@pytest.mark.parametrize('prefix', ['model.', ''])
def test_the_reference_s_own_tuned_file_loads(tmp_path, prefix):
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    config, ckpt, tuned = _files(tmp_path)
    entries = checkpoint.tuned_entries(tuned)
    path = str(tmp_path / 'spt.ckpt')
    torch.save({'state_dict': {prefix + k: t.detach().clone() for k, t in entries.items()}}, path)
    assert set(checkpoint.load_tuned(path)) == set(entries)
    _same_model(utils.load_spt_model(ckpt, path, d_lora=16), tuned)


def test_tuned_files_are_held_to_the_model(tmp_path):
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    config, ckpt, tuned = _files(tmp_path)
    entries = {k: t.detach().clone() for k, t in checkpoint.tuned_entries(tuned).items()}
    path = str(tmp_path / 'spt.ckpt')
    torch.save({'state_dict': dict(entries, stray=torch.zeros(3))}, path)
    with pytest.raises(RuntimeError, match='stray'):
        utils.load_spt_model(ckpt, path, d_lora=16)
    # a prefix on some keys only is no prefix: the keys are then unexpected
    some = {('model.' + k if i % 2 else k): t for i, (k, t) in enumerate(entries.items())}
    torch.save({'state_dict': some}, path)
    with pytest.raises(RuntimeError, match='model\\.'):
        utils.load_spt_model(ckpt, path, d_lora=16)
    lora = next(k for k in entries if 'lora' in k)
    torch.save({'state_dict': {k: t for k, t in entries.items() if k != lora}}, path)
    with pytest.raises(RuntimeError, match=lora.replace('.', '\\.')):
        utils.load_spt_model(ckpt, path, d_lora=16)
    torch.save({'config': config, 'tuned': {'format': 7}, 'state_dict': entries}, path)
    with pytest.raises(RuntimeError, match='format'):
        utils.load_spt_model(ckpt, path, d_lora=16)
    torch.save([1, 2], path)
    with pytest.raises(RuntimeError, match='not a naive_gpt checkpoint'):
        utils.load_spt_model(ckpt, path, d_lora=16)
