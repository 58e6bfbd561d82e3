"""LoRA routed FFNs on bf16 storage (grouped.RoutedLoRAFFNBf16 / RoutedLoRALLaMAFFNBf16, opt-in through
grouped.LORA_BF16): ms per call of forward + `sum().backward()` + AdamW on the LoRA tables and the router
(base weights frozen), three ways per shape and family -- bf16 fused, the bf16 per-block loop (the flag off:
today's path), fp32 fused.  Shapes: the reference's benchmark (d 2048, d_ff 8192, block 1024) and the FFN of
configs[2] (d 1024, d_ff 4096, block 1024), rank 16, 16 x 512 tokens.  Prints one JSON line.

    python tools/bench_routed_lora_bf16.py [--steps 10] [--warmup 3] [--only reference|configs2]
        [--family opt|llama] [--ways bf16_fused,bf16_loop,fp32_fused]
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
WAYS = {'bf16_fused': (torch.bfloat16, True, 'fused_bf16'), 'bf16_loop': (torch.bfloat16, False, 'torch_loop'),
        'fp32_fused': (torch.float32, False, 'fused')}


def timeit(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def make(family, d, dff, bs, r, dtype):
    torch.manual_seed(0)
    if family == 'opt':
        m = layers.LoRARoutedFFN(d_lora=r, block_size=bs, d_model=d, d_feedforward=dff, activation=nn.ReLU())
    else:
        m = layers.LoRARoutedLLaMaFFN(d_lora=r, block_size=bs, d_model=d, d_feedforward=dff, activation=nn.SiLU())
    with torch.no_grad():
        for name, p in m.named_parameters():
            if 'lora' in name:
                p.copy_(torch.randn_like(p) * 0.02)
            p.requires_grad_('lora' in name or 'router' in name)
    return m.cuda().to(dtype)


def run(m, x, flag, want_path, steps, warmup):
    grouped.LORA_BF16 = flag
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-5)

    def f():
        x.grad = None
        opt.zero_grad(set_to_none=True)
        m(x).float().sum().backward()
        opt.step()

    ext.reset_paths()
    ms = timeit(f, steps, warmup)
    assert set(ext.paths_taken('routed_ffn')) == {('routed_ffn', want_path)}, ext.paths_taken()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=sorted(SHAPES), default=None)
    ap.add_argument('--family', choices=['opt', 'llama'], default=None)
    ap.add_argument('--ways', default=','.join(WAYS))
    args = ap.parse_args()
    ways = args.ways.split(',')
    result = {'metric': 'routed_lora_ffn_bf16_ms_per_call', 'steps': args.steps, 'rank': 16,
              'tokens': 16 * 512, 'shapes': {}}
    for name, (d, dff, bs) in SHAPES.items():
        if args.only and name != args.only:
            continue
        for family in ('opt', 'llama'):
            if args.family and family != args.family:
                continue
            row = {'d': d, 'd_ff': dff, 'block': bs}
            x32 = torch.randn([16 * 512, d], device='cuda', requires_grad=True)
            for way in ways:
                dtype, flag, path = WAYS[way]
                m = make(family, d, dff, bs, 16, dtype)
                x = x32.detach().to(dtype).requires_grad_(True)
                row[way] = round(run(m, x, flag, path, args.steps, args.warmup), 3)
                del m, x
                torch.cuda.empty_cache()
            if 'bf16_fused' in row:
                for other in ('bf16_loop', 'fp32_fused'):
                    if other in row:
                        row['bf16_fused_vs_' + other] = round(row[other] / row['bf16_fused'], 3)
            result['shapes']['{}_{}'.format(name, family)] = row
            del x32
    grouped.LORA_BF16 = False
    print(json.dumps(result))


if __name__ == '__main__':
    main()
