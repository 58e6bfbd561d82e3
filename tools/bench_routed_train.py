"""Training step of the plain routed FFN: forward + `sum().backward()` + AdamW, ms per call, for the
dense Feedforward, RoutedFFN on the per-block loop and RoutedFFN on the grouped trainable path
(layers/sparse/grouped.py: RoutedFFNTrain, spt_grouped_gemm_wgrad).  Shapes: the reference's own
benchmark (test/layer/test_sparse_ffn.py: d 2048, d_ff 8192, block 1024, 16 x 512 tokens) and the
FFN of configs[2] (d 1024, d_ff 4096, block 1024, 16 x 512 tokens).  Prints one JSON line.

    python tools/bench_routed_train.py [--steps 10] [--warmup 3] [--only reference|configs2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'spt-proto_amd'))
import torch  # noqa: E402
from torch import nn  # noqa: E402
from naive_gpt import ext, layers  # noqa: E402
from naive_gpt.layers.sparse import grouped  # noqa: E402

SHAPES = {'reference': (2048, 8192, 1024), 'configs2': (1024, 4096, 1024)}


def timeit(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def train_step(m, x):
    opt = torch.optim.AdamW(m.parameters(), lr=1e-5)

    def f():
        opt.zero_grad(set_to_none=True)
        x.grad = None
        m(x).sum().backward()
        opt.step()
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=sorted(SHAPES), default=None)
    args = ap.parse_args()
    dev = 'cuda'
    result = {'metric': 'routed_ffn_train_ms_per_call', 'steps': args.steps, 'shapes': {}}
    for name, (d, dff, bs) in SHAPES.items():
        if args.only and name != args.only:
            continue
        torch.manual_seed(0)
        x = torch.randn([16, 512, d], device=dev, requires_grad=True)
        dense = layers.Feedforward(d_model=d, d_feedforward=dff, p_dropout=0.0, activation=nn.ReLU()).to(dev)
        routed = layers.RoutedFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=nn.ReLU()).to(dev)
        row = {'d': d, 'd_ff': dff, 'block': bs, 'tokens': 16 * 512}
        row['dense'] = timeit(train_step(dense, x), args.steps, args.warmup)
        grouped.TRAINABLE_WEIGHTS = False
        row['routed_loop'] = timeit(train_step(routed, x), args.steps, args.warmup)
        grouped.TRAINABLE_WEIGHTS = True
        ext.reset_paths()
        row['routed_grouped'] = timeit(train_step(routed, x), args.steps, args.warmup)
        assert set(ext.paths_taken('routed_ffn_plain')) == {('routed_ffn_plain', 'grouped_trainable')}
        row['grouped_vs_loop'] = row['routed_loop'] / row['routed_grouped']
        row = {k: round(v, 3) if isinstance(v, float) else v for k, v in row.items()}
        result['shapes'][name] = row
        del dense, routed, x
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
