"""SparseTuner.save / resume on the GPU: tuner A takes two training steps and saves, tuner B resumes from
the same base checkpoint; their states are equal entry by entry, and one further step from those equal
states agrees within the run-to-run bound test_model_step_ignores_what_its_buffers_held grants the
attention backward's float atomics (1e-5 of scale).  One step only: beyond it the 1e-7 differences
flip PQ codes and top-k choices, and two runs of ONE tuner part ways as well."""
import pytest
import torch

import test_gpu_poisoned_buffers as suite
from test_tuner_state import _equal_states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n_accumulate', [1, 2])
@pytest.mark.parametrize('kind', ['opt', 'llama'])
def test_resumed_tuner_takes_the_step_the_saved_one_takes(kind, n_accumulate, tmp_path):
    from naive_gpt import ext, utils
    from naive_gpt.utils import checkpoint
    torch.manual_seed(0)
    config = dict(suite.STEP_CONFIG)
    ckpt = str(tmp_path / (kind + '-toy.ckpt'))
    checkpoint.save_checkpoint(ckpt, config, checkpoint.build_model(kind, config))
    gen = suite._gen(40)
    batches = [torch.randint(0, config['vocab_size'], [suite.STEP_BATCH, config['max_length'] + 2], generator=gen).cuda()
               for _ in range(3)]
    a = utils.SparseTuner.from_checkpoint(ckpt, device='cuda', n_accumulate=n_accumulate)
    b = None
    try:
        for name, p in a.model.named_parameters():
            if name.endswith('lora.right.weight'):          # a fresh adapter is the identity
                p.data.copy_(0.05 * torch.randn(p.shape, generator=gen).cuda())
        ext.reset_paths()
        for batch in batches[:2]:
            a.training_step(batch)
        assert {k[1] for k in ext.paths_taken('head_loss')} == {'fused'}
        assert a._micro == 2 and a._flat is not None
        path = str(tmp_path / 'run.state')
        a.save(path)
        b = utils.SparseTuner.resume(ckpt, path, device='cuda', n_accumulate=n_accumulate)
        assert b._flat is not None
        sa, sb = a.state_dict(), b.state_dict()
        _equal_states(sa, sb, 'resumed')
        assert set(sa['step'].values()) == {2 // n_accumulate}
        assert any(bool(t.abs().sum() > 0) for t in sa['exp_avg'].values())
        # step 3: a whole step, n_accumulate micro-batches of the same batch
        for _ in range(n_accumulate):
            la, lb = a.training_step(batches[2]), b.training_step(batches[2])
            print('resume {} n_accumulate={}: loss {:.7f} / {:.7f}'.format(kind, n_accumulate, float(la), float(lb)))
            suite._close(lb, la, 'loss of step 3', rtol=1e-5)
        assert a.state_dict()['step'] == b.state_dict()['step']
        worst = 0.0
        for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
            if p.requires_grad:
                worst = max(worst, float((p - q).detach().abs().max() / p.detach().abs().max().clamp_min(1e-30)))
                suite._close(q, p, n + ' after step 3', rtol=1e-5)
        print('resume {} n_accumulate={}: largest parameter difference {:.2e} of scale'.format(kind, n_accumulate, worst))
    finally:
        a.release()
        if b is not None:
            b.release()


def test_state_reads_the_same_from_the_capturable_form_and_a_captured_tuner_refuses_to_load(tmp_path):
    """lr and step live in device tensors once the optimiser is capturable: the state holds them as plain
    values all the same, saving from a captured tuner works, loading into one says what to do instead."""
    from naive_gpt import utils
    from naive_gpt.utils import checkpoint
    kind = 'opt'
    torch.manual_seed(0)
    config = dict(suite.STEP_CONFIG)
    model = utils.upgrade_sparse(checkpoint.build_model(kind, config), d_lora=16).cuda()
    gen = suite._gen(41)
    batch = torch.randint(0, config['vocab_size'], [suite.STEP_BATCH, config['max_length'] + 2], generator=gen).cuda()
    a = utils.SparseTuner(model)
    try:
        a.capture(batch.shape, warmup=1, example=batch)
        a.training_step(batch)
        a.end_epoch()
        state = a.state_dict()
        assert isinstance(state['lr'], float) and abs(state['lr'] - 0.9e-4) < 1e-10
        steps = set(state['step'].values())             # the warm-up step and the replay (a capture runs nothing)
        assert len(steps) == 1 and min(steps) >= 2
        taken = float(min(steps))
        assert state['last_epoch'] == 1
        a.save(str(tmp_path / 'captured.state'))
        with pytest.raises(RuntimeError, match='before capturing'):
            a.load_state_dict(state)
        # into the capturable form before a capture: lr and step land in its device tensors
        a._graph = None
        a.use_capturable_optimizer()
        a.load_state_dict(state)
        group = a.optimizer.param_groups[0]
        assert torch.is_tensor(group['lr']) and abs(float(group['lr']) - 0.9e-4) < 1e-10
        entry = a.optimizer.state[a._flat]
        assert torch.is_tensor(entry['step']) and entry['step'].is_cuda and float(entry['step']) == taken
        _equal_states(state, a.state_dict(), 'capturable')
    finally:
        a.release()
