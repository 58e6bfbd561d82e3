"""SparseTuner.state_dict / load_state_dict / save / resume (utils/tuning.py): a run carried over a
process boundary takes the step it would have taken.  CPU only: gradients are injected, so no
kernel runs; the GPU twin (whole training steps, every optimiser form) is test_gpu_resume.py."""
import copy

import pytest
import torch

CONFIG = dict(d_model=128, n_heads=2, n_layers=1, max_length=64, vocab_size=96, d_feedforward=512, p_dropout=0.0)


def _tuner(n_accumulate=1, **kwargs):
    from naive_gpt import models, utils
    torch.manual_seed(0)
    model = utils.upgrade_sparse(models.OPTModel(**CONFIG), d_lora=16)
    gen = torch.Generator().manual_seed(1)
    for name, p in model.named_parameters():
        if name.endswith('lora.right.weight'):          # a fresh adapter is the identity
            p.data.copy_(0.05 * torch.randn(p.shape, generator=gen))
    return utils.SparseTuner(model, n_accumulate=n_accumulate, **kwargs)


def _inject(tuner, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in tuner.params:
        p.grad = torch.randn(p.shape, generator=gen)


def _moments(tuner):
    state = tuner.state_dict()
    return state['exp_avg'], state['exp_avg_sq'], state['step']


def _equal_states(a, b, what=''):
    assert set(a) == set(b)
    for key in a:
        if isinstance(a[key], dict):
            assert set(a[key]) == set(b[key]), (what, key)
            for name in a[key]:
                x, y = a[key][name], b[key][name]
                assert torch.equal(x, y) if torch.is_tensor(x) else x == y, (what, key, name)
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


def test_state_holds_what_the_issue_lists_and_no_frozen_weight():
    tuner = _tuner()
    _inject(tuner, 1)
    tuner.apply_gradients()
    state = tuner.state_dict()
    model = tuner.model
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    buffers = {n for n in model.state_dict() if n not in frozen and n not in trainable}
    assert frozen and trainable and buffers
    assert set(state['model']) == trainable | buffers
    assert set(state['exp_avg']) == set(state['exp_avg_sq']) == set(state['step']) == trainable
    assert all(t.device.type == 'cpu' for t in state['model'].values())
    assert set(state['step'].values()) == {1}
    assert state['format'] == 1 and state['lr'] == 1e-4 and state['betas'] == (0.9, 0.999)
    assert state['eps'] == 1e-8 and state['weight_decay'] == 1e-1 and state['gamma'] == 0.9
    assert state['last_epoch'] == 0 and state['_micro'] == 0 and state['n_accumulate'] == 1
    assert state['clip_norm'] == 1.0 and state['aux_weight'] == 1e-2


def test_saved_and_loaded_tuner_takes_the_same_next_step(tmp_path):
    a = _tuner()
    for seed in (1, 2):
        _inject(a, seed)
        a.apply_gradients()
    a.end_epoch()
    path = str(tmp_path / 'state.pt')
    a.save(path)
    b = _tuner()
    with torch.no_grad():
        for p in b.params:              # B does not start where A is
            p.add_(0.25)
    views = [p.data_ptr() for p in b.params]
    b.load_state_dict(torch.load(path, map_location='cpu', weights_only=True))
    assert [p.data_ptr() for p in b.params] == views, 'loading re-pointed a parameter'
    assert b._flat is not None and a._flat is not None
    b._check_flat_views()
    assert [p.data_ptr() for p in b.params] == views
    _equal_states(a.state_dict(), b.state_dict(), 'after load')
    for t in (a, b):
        _inject(t, 3)
        t.apply_gradients()
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n
    (ma, va, sa), (mb, vb, sb) = _moments(a), _moments(b)
    assert set(sa.values()) == {3} and sa == sb
    for n in ma:
        assert torch.equal(ma[n], mb[n]) and torch.equal(va[n], vb[n]), n
    for t in (a, b):
        t.end_epoch()
    assert a.lr == b.lr == pytest.approx(1e-4 * 0.81)
    assert a.scheduler.last_epoch == b.scheduler.last_epoch == 2
    assert a.scheduler.get_last_lr() == b.scheduler.get_last_lr()


def test_state_reads_the_same_from_the_flat_and_the_per_parameter_form(monkeypatch):
    from naive_gpt import utils
    a = _tuner()
    _inject(a, 1)
    a.apply_gradients()
    state = a.state_dict()
    monkeypatch.setattr(utils.SparseTuner, 'FLAT_LIMIT', 0)
    b = _tuner()
    assert b._flat is None
    b.load_state_dict(copy.deepcopy(state))
    _equal_states(state, b.state_dict(), 'flat -> per parameter')
    # a parameter that missed a step has a step count of its own: the flat form gives way
    uneven = copy.deepcopy(state)
    first = sorted(uneven['step'])[0]
    uneven['step'][first] = 0
    monkeypatch.undo()
    c = _tuner()
    assert c._flat is not None
    c.load_state_dict(uneven)
    assert c._flat is None
    _equal_states(uneven, c.state_dict(), 'uneven steps')


def test_a_state_before_the_first_step_loads():
    a, b = _tuner(), _tuner()
    state = a.state_dict()
    assert set(state['step'].values()) == {0}
    b.load_state_dict(state)
    for t in (a, b):
        _inject(t, 5)
        t.apply_gradients()
    for p, q in zip(a.params, b.params):
        assert torch.equal(p, q)


def test_refusals():
    a = _tuner(n_accumulate=2)
    a._micro = 1
    with pytest.raises(RuntimeError, match='micro-batches'):
        a.state_dict()
    a._micro = 2
    state = a.state_dict()
    b = _tuner(n_accumulate=2)
    names = sorted(state['exp_avg'])

    mid = copy.deepcopy(state)
    mid['_micro'] = 3
    with pytest.raises(ValueError, match='between the micro-batches'):
        b.load_state_dict(mid)

    renamed = copy.deepcopy(state)
    for key in ('exp_avg', 'exp_avg_sq', 'step'):
        renamed[key][names[0] + '_old'] = renamed[key].pop(names[0])
    with pytest.raises(ValueError, match=names[0]):
        b.load_state_dict(renamed)

    renamed = copy.deepcopy(state)
    renamed['model'][names[1] + '_old'] = renamed['model'].pop(names[1])
    with pytest.raises(ValueError, match=names[1]):
        b.load_state_dict(renamed)

    many = copy.deepcopy(state)
    for n in names[:6]:
        del many['model'][n]
    with pytest.raises(ValueError) as err:
        b.load_state_dict(many)
    assert sum(n in str(err.value) for n in names[:6]) == 4, 'up to four keys are named'

    shaped = copy.deepcopy(state)
    shaped['model'][names[0]] = torch.zeros([3])
    with pytest.raises(ValueError, match='shapes differ'):
        b.load_state_dict(shaped)
    shaped = copy.deepcopy(state)
    shaped['exp_avg_sq'][names[0]] = torch.zeros([3])
    with pytest.raises(ValueError, match='shapes differ'):
        b.load_state_dict(shaped)

    with pytest.raises(ValueError, match='n_accumulate'):
        _tuner(n_accumulate=1).load_state_dict(state)
    with pytest.raises(ValueError, match='format'):
        b.load_state_dict({'format': 99})
    # nothing was written by any refused load
    _equal_states(b.state_dict(), _tuner(n_accumulate=2).state_dict(), 'after the refusals')

    b._graph = object()         # a captured tuner
    with pytest.raises(RuntimeError, match='before capturing'):
        b.load_state_dict(state)
    b._graph = None


@pytest.mark.parametrize('frozen_fp16', [False, True])
def test_resume_from_the_base_checkpoint(tmp_path, frozen_fp16):
    from naive_gpt import models, utils
    torch.manual_seed(0)
    ckpt = str(tmp_path / 'opt-tiny.ckpt')
    base = models.OPTModel(**CONFIG)
    with torch.no_grad():
        for p in base.parameters():         # a base that was trained in halves: fp16 storage is exact
            p.copy_(p.half().float())
    utils.save_checkpoint(ckpt, CONFIG, base)
    a = utils.SparseTuner.from_checkpoint(ckpt, n_accumulate=2)
    for seed in (1, 2):
        _inject(a, seed)
        a.apply_gradients()
    path = str(tmp_path / 'run.state')
    a.save(path)
    b = utils.SparseTuner.resume(ckpt, path, n_accumulate=2, frozen_fp16=frozen_fp16)
    _equal_states(a.state_dict(), b.state_dict(), 'resumed')
    halves = [n for n, p in b.model.named_parameters() if p.dtype == torch.float16]
    assert bool(halves) == frozen_fp16 and (b.frozen_fp16_report is not None) == frozen_fp16
    assert not set(halves) & set(b.state_dict()['model'])
    with pytest.raises(ValueError, match='n_accumulate'):
        utils.SparseTuner.resume(ckpt, path)
