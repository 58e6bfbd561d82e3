"""bf16 routed FFN on the grouped matrix-core path (spt_grouped_gemm_bf16 / _wgrad_bf16): ms per call
of forward + `sum().backward()` (+ AdamW for the trainable rows), three ways per shape -- bf16 grouped,
the bf16 per-block loop (trainable weights: their path without grouped.TRAINABLE_WEIGHTS; frozen weights:
the grouped gate forced shut), fp32 grouped -- for frozen (forward + dX) and trainable weights.  Shapes: the reference's benchmark (d 2048, d_ff 8192, block
1024) and the FFN of configs[2] (d 1024, d_ff 4096, block 1024), 16 x 512 tokens.  Prints one JSON line.

    python tools/bench_routed_bf16.py [--steps 10] [--warmup 3] [--only reference|configs2]
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
from naive_gpt.layers.sparse import feedforward, grouped  # noqa: E402

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


def step_fn(m, x, train):
    opt = torch.optim.AdamW(m.parameters(), lr=1e-5) if train else None

    def f():
        x.grad = None
        if opt:
            opt.zero_grad(set_to_none=True)
        m(x).float().sum().backward()
        if opt:
            opt.step()
    return f


def run(m, x, train, want_path, steps, warmup):
    for p in m.parameters():
        p.requires_grad_(train)
    ext.reset_paths()
    ms = timeit(step_fn(m, x, train), steps, warmup)
    assert set(ext.paths_taken('routed_ffn_plain')) == {('routed_ffn_plain', want_path)}, ext.paths_taken()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=sorted(SHAPES), default=None)
    args = ap.parse_args()
    result = {'metric': 'routed_ffn_bf16_ms_per_call', 'steps': args.steps, 'shapes': {}}
    for name, (d, dff, bs) in SHAPES.items():
        if args.only and name != args.only:
            continue
        torch.manual_seed(0)
        m32 = layers.RoutedFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=nn.ReLU()).cuda()
        m16 = layers.RoutedFFN(d_model=d, d_feedforward=dff, block_size=bs, activation=nn.ReLU()).cuda().bfloat16()
        x32 = torch.randn([16 * 512, d], device='cuda', requires_grad=True)
        x16 = x32.detach().bfloat16().requires_grad_(True)
        row = {'d': d, 'd_ff': dff, 'block': bs, 'tokens': 16 * 512}
        # frozen base weights (forward + dX); their loop row has the grouped gate forced shut
        grouped.TRAINABLE_WEIGHTS = False
        row['frozen_bf16_grouped'] = run(m16, x16, False, 'grouped_bf16', args.steps, args.warmup)
        gate = feedforward._grouped_usable
        feedforward._grouped_usable = lambda *a: False
        try:
            row['frozen_bf16_loop'] = run(m16, x16, False, 'torch_loop', args.steps, args.warmup)
        finally:
            feedforward._grouped_usable = gate
        row['frozen_fp32_grouped'] = run(m32, x32, False, 'grouped', args.steps, args.warmup)
        row['train_bf16_loop'] = run(m16, x16, True, 'torch_loop', args.steps, args.warmup)
        grouped.TRAINABLE_WEIGHTS = True
        row['train_bf16_grouped'] = run(m16, x16, True, 'grouped_trainable_bf16', args.steps, args.warmup)
        row['train_fp32_grouped'] = run(m32, x32, True, 'grouped_trainable', args.steps, args.warmup)
        row['train_bf16_grouped_vs_loop'] = row['train_bf16_loop'] / row['train_bf16_grouped']
        row['frozen_bf16_grouped_vs_loop'] = row['frozen_bf16_loop'] / row['frozen_bf16_grouped']
        row['train_bf16_vs_fp32_grouped'] = row['train_fp32_grouped'] / row['train_bf16_grouped']
        row['frozen_bf16_vs_fp32_grouped'] = row['frozen_fp32_grouped'] / row['frozen_bf16_grouped']
        result['shapes'][name] = {k: round(v, 3) if isinstance(v, float) else v for k, v in row.items()}
        del m32, m16, x32, x16
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
