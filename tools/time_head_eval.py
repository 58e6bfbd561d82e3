"""The head part of `SparseTuner.validation_step` -- from the head's input h to the loss and the [B, B]
answer predictions -- on the fused evaluation head (layers/tuning/head_loss.py: lm_head_eval,
csrc/head_loss.hip: spt_cross_entropy_eval) against the library expression it replaces (the LoRA head's
[T, V] logits, nn.CrossEntropyLoss, argmax over the gathered rows), which is what the step ran before the
fused head existed.  Default: the OPT-1.3B head, V 50272, d 2048, rank 16, 16 x 2046 tokens.

The two legs alternate inside one process after a warm-up of both, each leg `--inner` calls between two
device events, every round runs each side twice; the spread is the larger difference between the medians
of a side's first and second legs.  Peak allocation: the rise of torch.cuda.max_memory_allocated() over
one call of each side, h and the head's weights excluded.  The losses and the predictions of both sides
are compared on the timed inputs.  Prints one JSON line.

    python tools/time_head_eval.py [--vocab 50272] [--d 2048] [--batch 16] [--seq 2046] [--inner 5] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'spt-proto_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--vocab', type=int, default=50272)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--rank', type=int, default=16)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--seq', type=int, default=2046)
    ap.add_argument('--max_rows', type=int, default=8192)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    import torch
    from torch import nn
    from naive_gpt import ext, layers
    from naive_gpt.layers.tuning import head_loss
    assert torch.cuda.is_available(), 'time_head_eval.py measures on the GPU'
    ext.load_library()
    torch.manual_seed(0)
    B, S, V, d = args.batch, args.seq, args.vocab, args.d
    head = layers.LoRALinear.from_pretrained(args.rank, nn.Linear(d, V, bias=False)).cuda()
    with torch.no_grad():
        head.lora.right.weight.normal_(0.0, 0.02)
    gen = torch.Generator().manual_seed(1)
    h = torch.randn([B, S, d], generator=gen).cuda()
    target = torch.randint(0, V, [B, S], generator=gen).cuda()
    position = torch.randint(2, S + 2, [B], generator=gen).cuda()
    loss_fn = nn.CrossEntropyLoss()
    assert head_loss.eval_usable(head, h)

    @torch.no_grad()
    def fused():
        loss, top = head_loss.lm_head_eval(head, h, target, max_rows=args.max_rows)
        return loss, top.view(B, S)[:, position - 2].long()

    @torch.no_grad()
    def library():
        output = head(h)
        loss = loss_fn(output.flatten(end_dim=-2), target=target.flatten())
        return loss, torch.argmax(output[:, position - 2, :], dim=-1)

    sides = {'fused': fused, 'library': library}
    outs, peak = {}, {}
    for name, fn in sides.items():                 # warm-up (first use re-homes the head's weight), then the peak
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        outs[name] = fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    rel = abs(float(outs['fused'][0]) - float(outs['library'][0])) / abs(float(outs['library'][0]))
    agree = float((outs['fused'][1] == outs['library'][1]).float().mean())

    def leg(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.inner):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / args.inner

    legs = {name: ([], []) for name in sides}
    for _ in range(args.rounds):
        for half in (0, 1):
            for name, fn in sides.items():
                legs[name][half].append(leg(fn))
    ms = {name: statistics.median(a + b) for name, (a, b) in legs.items()}
    spread = max(abs(statistics.median(a) - statistics.median(b)) for a, b in legs.values())
    print(json.dumps({
        'what': 'head part of validation_step', 'device': torch.cuda.get_device_name(0),
        'vocab': V, 'd_model': d, 'rank': args.rank, 'tokens': B * S, 'max_rows': args.max_rows,
        'chunks': len(head_loss._chunk_bounds(B * S, args.max_rows)) - 1,
        'fused_ms': round(ms['fused'], 3), 'library_ms': round(ms['library'], 3), 'spread_ms': round(spread, 3),
        'fused_peak_bytes': peak['fused'], 'library_peak_bytes': peak['library'],
        'one_logits_tensor_bytes': B * S * V * 4,
        'loss_rel_diff': rel, 'grid_predictions_equal': agree, 'inner': args.inner, 'rounds': args.rounds}))


if __name__ == '__main__':
    main()
