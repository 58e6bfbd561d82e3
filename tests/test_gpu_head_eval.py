"""The fused evaluation head: spt_cross_entropy_eval through ext.cross_entropy_grad_(evaluate=True)
(csrc/head_loss.hip), layers/tuning/head_loss.py: lm_head_eval, and SparseTuner.validation_step on it.

Kernel: the row loss against fp32_contract.head_loss_refs on head_loss_inputs, within that function's
bound (the kernel keeps the gradient kernel's expressions and trees); the argmax against fp64; planted
rows; pad columns holding +inf and NaN; the logits bit for bit what they were.  Then the poison, guard-band
and graph-replay tiers on two cases of the new mode, and the layer and the tuner against the library head.
"""
import functools

import pytest
import torch
from torch import nn

import fp32_contract as C
import test_gpu_graph_replay as tier
import test_gpu_guard_bands as bands
import test_gpu_poisoned_buffers as suite
from poison import same_bits
from test_gpu_poisoned_buffers import DET, Case

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# ld <= 32768: the row stays in registers between the two passes; above: it is read twice
SHAPES = [(7, 8), (1000, 1056), (32768, 32768), (32772, 32772), (50272, 50304)]
ONE_ROW = 5         # head_loss_inputs needs two rows or more for its spreads: the one-row case is this
                    # (counted) row of the 33-row inputs, with the bound of the same row


@functools.lru_cache(maxsize=None)
def _reference(V, ld):
    """(inputs, refs, fp64 argmax) of the 33-row case, computed once per shape and left unchanged."""
    inp = C.head_loss_inputs(V, ld, seed=V)
    refs = C.head_loss_refs(inp)
    return inp, refs['loss'], _first_argmax(inp['logits'][:, :V])


def _first_argmax(z):
    z = z.double()
    at = torch.arange(z.size(1)).expand_as(z)
    return torch.where(z == z.max(-1, keepdim=True).values, at, z.size(1)).min(-1).values


def _evaluate(logits, V, target, **kwargs):
    from naive_gpt import ext
    before = logits.clone()
    loss, top = ext.cross_entropy_grad_(logits, V, target, None, evaluate=True, **kwargs)
    torch.cuda.synchronize()
    assert same_bits(logits, before), 'the evaluation mode wrote the logits'
    assert loss.dtype == torch.float32 and top.dtype == torch.int32 and loss.shape == top.shape == (logits.size(0),)
    return loss, top


@pytest.mark.parametrize('rows', [1, 33])
@pytest.mark.parametrize('V,ld', SHAPES)
def test_row_loss_within_the_head_loss_bound_and_argmax_exact(V, ld, rows):
    inp, (ref, bound), want_top = _reference(V, ld)
    pick = slice(ONE_ROW, ONE_ROW + 1) if rows == 1 else slice(None)
    assert rows == 33 or int(inp['target'][ONE_ROW]) >= 0
    target = inp['target'][pick].to(DEV)
    outs = []
    for pad in (float('inf'), float('nan')):
        logits = inp['logits'][pick].clone()
        logits[:, V:] = pad                         # columns the head's GEMM leaves unwritten
        loss, top = _evaluate(logits.to(DEV), V, target)
        ratios = C.check(dict(loss=loss), {'loss': (ref[pick], bound[pick])}, 'eval head V={} rows={} pad={}'.format(V, rows, pad))
        print('eval head V={} ld={} rows={} pad={}: loss at {:.3f} of its bound'.format(V, ld, rows, pad, ratios['loss']))
        assert torch.equal(top.cpu().long(), want_top[pick]), 'argmax differs from fp64'
        outs.append((loss, top))
    assert same_bits(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'the pad columns reached a result'
    if rows == 33:
        assert (outs[0][0][::4] == 0).all() and (outs[0][0][1::4] != 0).all()        # every 4th target is ignored


@pytest.mark.parametrize('V,ld', [(1000, 1056), (32772, 32776), (7, 8)])
def test_planted_rows(V, ld):
    gen = torch.Generator().manual_seed(V)
    names = ['max_first', 'max_last', 'tie', 'flat', 'ignored', 'above_range', 'below_range', 'own_ignore_index',
             'nan', 'all_nan', 'random', 'random2']
    R = len(names)
    z = torch.randn([R, V], generator=gen)
    ties = sorted({8 % V, (1030 if V > 1030 else 500) % V, V - 1})   # (V > 1030: column 8 sits in a higher thread than 1030)
    row = {n: i for i, n in enumerate(names)}
    z[row['max_first'], 0] = 9.0
    z[row['max_last'], V - 1] = 9.0
    z[row['tie'], ties] = 9.0
    z[row['flat']] = -2.5
    z[row['nan'], 3] = float('nan')
    z[row['all_nan']] = float('nan')
    target = torch.randint(0, V, [R], generator=gen)
    target[row['ignored']] = 4 % V
    target[row['above_range']] = V + 5
    target[row['below_range']] = -3
    target[row['own_ignore_index']] = 4 % V
    target[row['nan']] = 1
    target[row['ignored']] = -100
    logits = torch.full([R, ld], float('inf'))
    logits[:, :V] = z
    # under ignore_index = 4 % V the rows planted with that target are ignored, and -100 is merely out of
    # range: ignored as well
    for ignore in (-100, 4 % V):
        tgt = target
        loss, top = _evaluate(logits.to(DEV), V, tgt.to(DEV), ignore_index=ignore)
        loss, top = loss.cpu(), top.cpu().long()
        assert ((top >= 0) & (top < V)).all()
        assert top[row['max_first']] == 0 and top[row['max_last']] == V - 1
        assert top[row['tie']] == ties[0] and top[row['flat']] == 0 and top[row['all_nan']] == 0
        finite = [i for n, i in row.items() if n not in ('nan', 'all_nan')]
        assert torch.equal(top[finite], _first_argmax(z[finite]))
        nan_row = z[row['nan']].clone()
        nan_row[3] = float('-inf')
        assert top[row['nan']] == _first_argmax(nan_row[None])[0], 'a NaN won or hid the maximum'
        counted = (tgt != ignore) & (tgt >= 0) & (tgt < V)
        for n in ('nan', 'all_nan'):            # a counted row holding NaN: NaN; not counted: 0 as any other
            assert bool(torch.isnan(loss[row[n]])) == bool(counted[row[n]]), n
        assert counted[row['nan']]
        for n in ('ignored', 'above_range', 'below_range'):
            assert not counted[row[n]] and loss[row[n]] == 0
        assert (loss[~counted] == 0).all()
        if ignore != -100:
            assert loss[row['own_ignore_index']] == 0
        live = [i for i in finite if counted[i]]
        want = torch.logsumexp(z[live].double(), -1) - z[live].double().gather(1, tgt[live][:, None])[:, 0]
        assert torch.allclose(loss[live].double(), want, rtol=1e-5, atol=1e-6), (loss[live], want)


def test_scale_is_optional_only_when_evaluating():
    from naive_gpt import ext
    logits = torch.zeros([2, 8], device=DEV)
    target = torch.zeros([2], dtype=torch.long, device=DEV)
    with pytest.raises((RuntimeError, AttributeError, TypeError)):
        ext.cross_entropy_grad_(logits, 7, target, None)
    loss, top = ext.cross_entropy_grad_(logits, 7, target, torch.ones(1, device=DEV), evaluate=True)
    assert loss.shape == (2,) and (top == 0).all() and (logits == 0).all()
    loss0, top0 = ext.cross_entropy_grad_(logits[:0], 7, target[:0], None, evaluate=True)
    assert loss0.numel() == 0 and top0.numel() == 0 and top0.dtype == torch.int32


# ---------------------------------------------------------------------------------------------------
# the harness tiers on the new mode: built as the registry's `_cross_entropy` case is

def _cross_entropy_eval(rows, V, ld):
    def build():
        from naive_gpt import ext
        gen = suite._gen(51 + V)
        z = suite._dev(3.0 * torch.randn([rows, V], generator=gen))
        target = suite._dev(torch.randint(0, V, [rows], generator=gen))
        target[::4] = -100
        buf = suite._dev(torch.full([rows, ld], 7.0))
        buf[:, :V] = z

        def call():
            loss, top = ext.cross_entropy_grad_(buf, V, target, None, evaluate=True)
            return loss, top, buf            # (the operand too: it must come back as it went in)

        def check(outs):
            loss, top, after = outs
            want = torch.nn.functional.cross_entropy(z.double(), target, reduction='none')
            suite._close(loss, want, 'loss rows', rtol=1e-5)
            assert (loss[::4] == 0).all(), 'ignored rows not exactly 0'
            assert torch.equal(top.long().cpu(), _first_argmax(z.cpu())), 'argmax'
            assert torch.equal(after[:, :V], z) and (after[:, V:] == 7.0).all(), 'the logits changed'
        return call, check
    return build


TIER_CASES = [Case('eval_ignored_rows_ragged_v', _cross_entropy_eval(33, 1001, 1056), DET),
              Case('eval_two_reads', _cross_entropy_eval(3, 32770, 32776), DET)]
TIER_PARAMS = [pytest.param(c, id=c.name) for c in TIER_CASES]


@pytest.mark.parametrize('case', TIER_PARAMS)
def test_eval_mode_ignores_what_its_buffers_held(case):
    suite.test_entry_ignores_what_its_buffers_held('cross_entropy_grad_', case)


@pytest.mark.parametrize('case', TIER_PARAMS)
def test_eval_mode_stays_inside_its_buffers(case):
    bands.test_entry_stays_inside_its_buffers('cross_entropy_grad_', case)


@pytest.mark.parametrize('case', TIER_PARAMS[:1])
def test_eval_mode_replayed_on_new_logits_and_targets_equals_eager(case):
    tier.test_entry_replayed_on_new_inputs_equals_eager('cross_entropy_grad_', case)


# ---------------------------------------------------------------------------------------------------
# the layer and the tuner: d 256, V 1000 (the head of test_gpu_head_loss), 4096 tokens in two chunks

D, V_HEAD, T_HEAD = 256, 1000, 4096
MARGIN = 1e-3       # relative top-2 margin above which an argmax is the same on any engine (the north-star bar)


def _margins(logits):
    top2 = logits.double().flatten(end_dim=-2).topk(2, dim=-1).values
    return (top2[:, 0] - top2[:, 1]) / top2[:, 0].abs()


def test_lm_head_eval_against_the_library_head():
    from naive_gpt.layers.tuning import head_loss
    from test_gpu_head_loss import _head
    head = _head(D, V_HEAD)
    gen = torch.Generator().manual_seed(2)
    # every token leans towards one class (12 x the unit row of the head's effective weight, the adapter's
    # low-rank part kept below the base's): the head's answer is known and its margin wide, on every row
    klass = torch.randint(0, V_HEAD, [T_HEAD], generator=gen)
    with torch.no_grad():
        head.lora.right.weight.mul_(0.1)
        w = (head.weight + head.lora.right.weight @ head.lora.left.weight.t()).cpu()
    x = (torch.randn([T_HEAD, D], generator=gen) + 12.0 * nn.functional.normalize(w[klass], dim=-1)).view(8, 512, D).to(DEV)
    target = torch.randint(0, V_HEAD, [8, 512], generator=gen).to(DEV)
    target[0, :7] = -100
    assert head_loss._chunk_bounds(T_HEAD, 2048) == [0, 2048, 4096]
    assert head_loss._chunk_bounds(T_HEAD, 8192) == [0, 4096] and head_loss._chunk_bounds(T_HEAD, 100) == [0, 2048, 4096]
    assert head_loss._chunk_bounds(6000, 2048) == [0, 3000, 6000] and head_loss._chunk_bounds(2049, 2048) == [0, 2049]
    before = head.weight.detach().clone()
    with torch.no_grad():
        for p in head.parameters():
            p.requires_grad_(False)             # tables that train nothing: evaluation takes them
        assert head_loss.eval_usable(head, x) and not head_loss.fused_usable(head, x)
        logits = head(x)
        want = nn.CrossEntropyLoss()(logits.flatten(end_dim=-2), target.flatten())
        for max_rows in (2048, 8192):
            loss, top = head_loss.lm_head_eval(head, x, target, max_rows=max_rows)
            assert loss.dim() == 0 and top.shape == (T_HEAD,) and top.dtype == torch.int32
            err = abs(float(loss) - float(want))
            print('lm_head_eval max_rows={}: loss {:.7f} library {:.7f} rel err {:.2e}'.format(
                max_rows, float(loss), float(want), err / abs(float(want))))
            assert err <= 1e-5 * abs(float(want))
            margins = _margins(logits)
            assert bool((margins > MARGIN).all()), 'rows under the margin: {}'.format(int((margins <= MARGIN).sum()))
            assert torch.equal(top.long(), logits.flatten(end_dim=-2).argmax(-1))
            assert torch.equal(top.long().cpu(), klass)
        nothing = torch.full_like(target, -100)
        assert torch.isnan(head_loss.lm_head_eval(head, x, nothing)[0]) and \
            torch.isnan(nn.CrossEntropyLoss()(logits.flatten(end_dim=-2), nothing.flatten()))
    assert torch.equal(head.weight.detach(), before)


def _validation_setup():
    from naive_gpt import models, utils
    torch.manual_seed(0)
    with torch.device('cuda'):
        model = models.OPTModel(d_model=D, n_heads=4, n_layers=1, max_length=512, vocab_size=V_HEAD,
                                d_feedforward=1024, p_dropout=0.0)
        model = utils.upgrade_sparse(model, d_lora=16, stages=('lora',))
    with torch.no_grad():
        model.lm_output.lora.right.weight.normal_(0.0, 0.05)
    tuner = utils.SparseTuner(model)
    tuner.EVAL_MAX_ROWS = 2048
    gen = torch.Generator().manual_seed(7)
    batch = torch.randint(3, V_HEAD, [8, 514], generator=gen).to(DEV)
    # The answer positions.  The model is causal: the logits that predict column p read columns < p only.
    # Ascending p, a column is taken when the LIBRARY head's top-2 margin there is ten times the bar on every
    # row (a random model's argmax is otherwise a coin toss somewhere in 64 cells), and the upper half of the
    # rows get the library head's own prediction as their answer, so that the accuracy grid holds right
    # answers and wrong ones.
    model.eval()
    position, p = [], 5
    with torch.no_grad():
        while len(position) < 8:
            logits = model(batch[:, 1:-1])
            wide = (_margins(logits).view(8, 512) > 10 * MARGIN).all(0)             # per output index p - 2
            p = next(q for q in range(p, 513) if bool(wide[q - 2]))
            batch[4:, p] = logits[4:, p - 2].argmax(-1)
            position.append(p)
            p += 40
    batch[:, 0] = torch.tensor(position, device=DEV)
    return tuner, batch


def test_validation_step_on_the_fused_head(monkeypatch):
    from naive_gpt import ext
    from naive_gpt.layers.tuning import head_loss
    tuner, batch = _validation_setup()
    model = tuner.model
    try:
        with torch.no_grad():
            logits = model(batch[:, 1:-1])
        position = batch[:, 0]
        cells = logits[:, position - 2, :]                              # the [B, B] grid's logits
        assert bool((_margins(cells) > MARGIN).all()), 'a scored cell of the grid is under the margin'
        ext.reset_paths()
        fused = tuner.validation_step(batch)
        assert ext.paths_taken('head_eval') == {('head_eval', 'fused'): 1}
        assert not model.training
        monkeypatch.setattr(head_loss, 'eval_usable', lambda head, x: False)
        ext.reset_paths()
        library = tuner.validation_step(batch)
        assert ext.paths_taken('head_eval') == {('head_eval', 'library'): 1}
        assert any('fused evaluation' in r for r in ext.fallback_reasons('head_eval', 'library'))
        monkeypatch.undo()
        plain = dict(zip(('logits', 'loss'), tuner.shared_step(batch[:, 1:-1], target=batch[:, 2:])))
        assert torch.equal(library['loss'], plain['loss']), 'the library path is no longer shared_step bit for bit'
        for key in ('loss', 'ppl'):
            err = abs(float(fused[key]) - float(library[key]))
            print('validation_step {}: fused {:.7f} library {:.7f} rel err {:.2e}'.format(
                key, float(fused[key]), float(library[key]), err / abs(float(library[key]))))
        assert abs(float(fused['loss']) - float(library['loss'])) <= 1e-5 * abs(float(library['loss']))
        assert abs(float(fused['ppl']) - float(library['ppl'])) <= 2e-5 * abs(float(library['ppl'])) * max(1.0, float(library['loss']))
        assert float(fused['accuracy']) == float(library['accuracy'])
        assert 0.4 <= float(fused['accuracy']) <= 0.6, 'the grid was planted half right'
        # a small batch keeps the library path, and says why
        ext.reset_paths()
        small = tuner.validation_step(batch[:2])
        assert ext.paths_taken('head_eval') == {('head_eval', 'library'): 1} and torch.isfinite(small['loss'])
    finally:
        tuner.release()


def test_fused_validation_allocates_less_than_one_logits_tensor(monkeypatch):
    """The head part of the fused validation_step (from the head's input to loss and argmaxes) raises the
    allocator's peak by less than one [T, V] fp32 tensor; the library head raises it by more than one."""
    from naive_gpt.layers.tuning import head_loss
    tuner, batch = _validation_setup()
    one_tensor = T_HEAD * V_HEAD * 4
    seen = {}
    inner = head_loss.lm_head_eval

    def measured(*args, **kwargs):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = inner(*args, **kwargs)
        torch.cuda.synchronize()
        seen['fused'] = torch.cuda.max_memory_allocated() - base
        seen['max_rows'] = kwargs.get('max_rows')
        return out

    try:
        tuner.validation_step(batch)                                   # (first use: the head's weight moves into padded storage)
        monkeypatch.setattr(head_loss, 'lm_head_eval', measured)
        tuner.validation_step(batch)
        assert seen['max_rows'] == 2048
        with torch.no_grad():
            h = tuner.model.hidden(batch[:, 1:-1])
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tuner.loss_fn(tuner.model.lm_output(h).flatten(end_dim=-2), target=batch[:, 2:].flatten())
            torch.cuda.synchronize()
            library = torch.cuda.max_memory_allocated() - base
        print('head part of validation_step, peak allocation: fused {} bytes, library {} bytes, one [T, V] fp32 tensor {}'.format(
            seen['fused'], library, one_tensor))
        assert seen['fused'] < one_tensor
        assert library > one_tensor
    finally:
        tuner.release()
