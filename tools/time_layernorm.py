"""Forward + backward of `fused_norm.add_norm` with an addend and a skip gradient, per model width, on
the fused add + norm kernels (csrc/layernorm.hip) against the op-by-op library expression that runs
where the kernels refuse a width (`fused_norm.usable` forced false: a separate addition, the library
norm, a separate addition of the skip gradient in the backward).  Rows: 16 x 512 and 2 x 2048.

Per width one child process under its own time limit; the first failure ends the run.  Inside a child
the two paths alternate, leg after leg, each leg `--inner` calls between two device events after a
warm-up of both; every round runs each side TWICE, and the spread is the larger difference between
the medians of a side's first and second legs.  A width is accepted when the library time exceeds the
fused time by more than that spread.  Achieved bytes per second come from the shapes (forward: read x
and r, write s and y; backward: read s, dy and the skip gradient, write dx: 8 rows d floats), printed
beside the same figure at d = 2048 as a per-byte yardstick.  `rms4096_wide` times the wave-per-row RMS
4096 kernel against the wide-row form of the same width (SPT_LAYERNORM_WIDE, read at every call).
Prints one JSON line.

    python tools/time_layernorm.py [--inner 50] [--rounds 10] [--limit 240] [--only 2560]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ((16, 512), (2, 2048))
# (name, d, rms): the new widths, then the yardstick and the width RMS had before
CASES = [('768_layernorm', 768, False), ('768_rms', 768, True), ('2560_layernorm', 2560, False),
         ('2560_rms', 2560, True), ('4096_layernorm', 4096, False), ('5120_layernorm', 5120, False),
         ('5120_rms', 5120, True), ('2048_layernorm', 2048, False), ('2048_rms', 2048, True),
         ('4096_rms', 4096, True), ('rms4096_wide', 4096, True)]


def child(name, d, rms, inner, rounds):
    sys.path.insert(0, os.path.join(ROOT, 'spt-proto_amd'))
    import torch
    from torch import nn
    from naive_gpt import ext, layers
    from naive_gpt.layers.basic import fused_norm
    assert torch.cuda.is_available(), 'time_layernorm.py measures on the GPU'
    dev = 'cuda'
    usable = fused_norm.usable
    wide_pair = name == 'rms4096_wide'
    out = {'d': d, 'norm': 'rms' if rms else 'layernorm', 'form': ext.layernorm_form(d, rms), 'rows': {}}
    for n, s in ROWS:
        torch.manual_seed(0)
        norm = (layers.LlamaRMSNorm(d) if rms else nn.LayerNorm(d)).to(dev)
        x = torch.randn([n, s, d], device=dev, requires_grad=True)
        r = torch.randn([n, s, d], device=dev, requires_grad=True)
        gs, gy = torch.randn([n, s, d], device=dev), torch.randn([n, s, d], device=dev)

        def step():
            x.grad = r.grad = None
            norm.zero_grad(set_to_none=True)
            a, b = fused_norm.add_norm(norm, x, r)
            torch.autograd.backward((a, b), (gs, gy))

        def side(first):
            """first: the fused kernels (wide pair: the wave-per-row kernel); else what they are compared with"""
            if wide_pair:
                os.environ['SPT_LAYERNORM_WIDE'] = '0' if first else '1'
                assert ext.layernorm_form(d, rms) == (1 if first else 4)
            else:
                fused_norm.usable = usable if first else (lambda *a, **k: False)

        def leg(first):
            side(first)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(inner):
                step()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) / inner * 1e3            # us per call

        for first in (True, False):                                  # warm-up, and which engine ran
            ext.reset_paths()
            side(first)
            for _ in range(5):
                step()
            torch.cuda.synchronize()
            want = 'kernel' if first or wide_pair else 'library'
            assert set(ext.paths_taken('norm')) == {('norm', want)}, ext.paths_taken('norm')
        legs = {(f, k): [] for f in (True, False) for k in (0, 1)}
        for _ in range(rounds):
            for k in (0, 1):
                for first in (True, False):
                    legs[(first, k)].append(leg(first))
        fused_norm.usable = usable
        os.environ.pop('SPT_LAYERNORM_WIDE', None)
        med = {key: statistics.median(v) for key, v in legs.items()}
        a = statistics.median(legs[(True, 0)] + legs[(True, 1)])
        b = statistics.median(legs[(False, 0)] + legs[(False, 1)])
        spread = max(abs(med[(True, 0)] - med[(True, 1)]), abs(med[(False, 0)] - med[(False, 1)]))
        nbytes = 8 * n * s * d * 4
        row = {'bytes': nbytes, 'spread_us': round(spread, 2)}
        if wide_pair:
            row.update(wave_per_row_us=round(a, 2), wide_us=round(b, 2))
        else:
            row.update(fused_us=round(a, 2), library_us=round(b, 2), fused_gbs=round(nbytes / a * 1e-3, 1),
                       library_gbs=round(nbytes / b * 1e-3, 1), accepted=bool(b - a > spread))
        out['rows']['{}x{}'.format(n, s)] = row
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--limit', type=int, default=240, help='seconds per width')
    ap.add_argument('--only', default=None, help='case names starting with this')
    ap.add_argument('--child', default=None)
    args = ap.parse_args()
    if args.child:
        name, d, rms = next(c for c in CASES if c[0] == args.child)
        return child(name, d, rms, args.inner, args.rounds)
    result = {'metric': 'add_norm_forward_backward_us', 'inner': args.inner, 'rounds': args.rounds, 'cases': {}}
    failed = None
    for name, d, rms in CASES:
        if args.only and not name.startswith(args.only):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), '--child', name, '--inner', str(args.inner),
               '--rounds', str(args.rounds)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            failed = '{}: no result within {} s'.format(name, args.limit)
            break
        if done.returncode != 0:
            failed = '{}: exit status {}: {}'.format(name, done.returncode, done.stderr.strip()[-400:])
            break
        result['cases'][name] = json.loads(done.stdout.strip().splitlines()[-1])
        print('[time_layernorm] {} {}'.format(name, result['cases'][name]['rows']), file=sys.stderr, flush=True)
    # the per-byte yardstick: each case's fused rate over the d = 2048 rate of the same norm and rows
    for name, case in result['cases'].items():
        yard = result['cases'].get('2048_' + case['norm'])
        for key, row in case['rows'].items():
            if yard and 'fused_gbs' in row:
                row['rate_vs_2048'] = round(row['fused_gbs'] / yard['rows'][key]['fused_gbs'], 3)
    if failed:
        result['stopped_at'] = failed          # nothing more is started on the GPU after a failure
    print(json.dumps(result))
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
