"""Golden vectors for TRAINING the plain routed FFNs, by IMPORTING THE REFERENCE (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_routed_train.py [reference checkout]

The reference's RoutedFFN (ReLU) and RoutedLLaMaFFN (SiLU) run as they are, on the CPU, in float64
from inputs and weights that are exact in float16 (stored so: the fixture stays small): forward, then `(y * w).sum().backward()`.  Stored: the inputs, the
state_dicts, y, and the gradients of x and of every FFN weight and bias; that the router's gradients
are None is recorded too (its probabilities only feed the top-k).  The inputs are drawn until every
token's top-k margin (k-th minus (k+1)-th router probability) exceeds 1e-4, so that fp32 routing on
the GPU cannot pick different blocks.

Output: tests/golden/routed_train.npz (data only; no reference source is copied).
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('SPT_REFERENCE', '/root/reference')

sys.dont_write_bytecode = True
sys.modules['naive_gpt.ext'] = types.ModuleType('naive_gpt.ext')          # (CUDA-only; not reached)
sys.modules['naive_gpt.loaders'] = types.ModuleType('naive_gpt.loaders')
sys.path.insert(0, REFERENCE)
import naive_gpt  # noqa: E402
from naive_gpt import layers  # noqa: E402

assert naive_gpt.__file__.startswith(os.path.abspath(REFERENCE))

D, DFF, BS, SHAPE = 32, 512, 64, (2, 150)
MARGIN = 1e-4


def margin(module, x, k):
    prob = module.router(x.reshape(-1, D)).detach()
    top = torch.sort(prob, dim=-1, descending=True).values
    return (top[:, k - 1] - top[:, k]).min().item()


def make(kind, seed):
    for attempt in range(100):
        torch.manual_seed(seed + 1000 * attempt)
        if kind == 'opt':
            m = layers.RoutedFFN(d_model=D, d_feedforward=DFF, block_size=BS, activation=nn.ReLU())
            k = m.n_blocks // 2
        else:
            m = layers.RoutedLLaMaFFN(d_model=D, d_feedforward=DFF, block_size=BS, activation=nn.SiLU())
            k = m.n_blocks // 4
        with torch.no_grad():                # a router with a spread worth the name
            m.router[0].weight.mul_(8.0)
            for p in m.parameters():
                p.copy_(p.half().float())
        x = torch.randn(SHAPE + (D,)).half().float()
        w = torch.randn(SHAPE + (D,)).half().float()
        m = m.double()
        x64 = x.double().requires_grad_(True)
        if margin(m, x64, k) > MARGIN:
            break
    else:
        raise RuntimeError('no input with a top-k margin above {}'.format(MARGIN))
    y = m(x64)
    (y * w.double()).sum().backward()
    out = {'x': x.half().numpy(), 'w': w.half().numpy(), 'y': y.detach().float().numpy(),
           'grad_x': x64.grad.float().numpy(), 'margin': np.float64(margin(m, x64, k))}
    for name, p in m.named_parameters():
        out['param.' + name] = p.detach().half().numpy()
        if name.startswith('router'):
            out['router_grad_is_none.' + name] = np.bool_(p.grad is None)
            assert p.grad is None, name
        else:
            out['grad.' + name] = p.grad.float().numpy()
    return {kind + '.' + key: v for key, v in out.items()}


def main():
    data = {}
    data.update(make('opt', 11))
    data.update(make('llama', 23))
    path = os.path.join(HERE, 'routed_train.npz')
    np.savez_compressed(path, **data)
    print('wrote', path, os.path.getsize(path), 'bytes;',
          'margins', data['opt.margin'], data['llama.margin'])


if __name__ == '__main__':
    main()
