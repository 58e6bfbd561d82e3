"""Time and weigh the sparse attention layer with grouped key/value heads (GQA): the kernels that
read the kv head in place against the expanded form (SPT_GQA_EXPAND=1), and one MHA shape that must
not have become slower.

    python tools/bench_gqa.py [--label NAME] [--out profiles/gqa_attention.json] [--reps 30]
                              [--mha-only] [--package DIR]

One run appends {label, device, mha, gqa} to the `runs` list of the output file.  Per shape and form:
the median over `--reps` forward + backward passes of SparseVanillaAttentionV2 (PQ encode, lookup,
attention node, its backward), each timed with a pair of HIP events after three warm-up passes; the
bytes held between forward and backward on copies of q, k, v (they stand for the projections' outputs:
what a model keeps per layer until its backward); and the peak above the inputs during that pass
(torch.cuda.max_memory_allocated).

`--mha-only` with `--package DIR` (a checkout's spt-proto_amd with its built lib) times the MHA shape
on another commit: it uses nothing that commit may lack.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--label', default='this')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gqa_attention.json'))
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--mha-only', action='store_true')
ap.add_argument('--package', default=os.path.join(ROOT, 'spt-proto_amd'))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package))
import torch  # noqa: E402
from naive_gpt import ext, layers  # noqa: E402

GQA_SHAPES = [(1, 32, 8, 128, 2048), (2, 32, 4, 64, 2048)]       # (N, H, kv, E, S): LLaMA-3-8B / TinyLlama heads
MHA_SHAPE = (16, 16, 16, 64, 512)                                 # BASELINE configs[2]
dev = 'cuda'


def measure(N, H, KV, E, S, expand):
    os.environ['SPT_GQA_EXPAND'] = '1' if expand else '0'
    torch.manual_seed(0)
    attn = layers.SparseVanillaAttentionV2(d_head=E, d_codeword=8, n_codewords=16, p_dropout=0.0).to(dev)
    q = torch.randn([N, S, H, E], device=dev, requires_grad=True)
    k, v = (torch.randn([N, S, KV, E], device=dev, requires_grad=True) for _ in range(2))
    w = torch.randn([N, S, H, E], device=dev)

    def step():
        q.grad = k.grad = v.grad = None
        attn(q, k, v, attn_mask=None).backward(w)

    ext.reset_paths()
    for _ in range(3):
        step()
    paths = sorted(p for _, p in ext.paths_taken('attention'))
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    q.grad = k.grad = v.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    # (copies stand for the projections' outputs, which nothing but the node keeps alive: of the
    # inputs' own tensors the measurement would not see which form holds on to which)
    y = attn(q.clone(), k.clone(), v.clone(), attn_mask=None)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base - y.numel() * y.element_size()
    y.backward(w)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del y
    times.sort()
    return {'shape': {'N': N, 'H': H, 'kv': KV, 'E': E, 'S': S}, 'form': 'expanded' if expand else 'kernel',
            'paths': paths, 'fwd_bwd_us_median': statistics.median(times), 'fwd_bwd_us_min': times[0],
            'fwd_bwd_us_p90': times[int(0.9 * (len(times) - 1))], 'held_bytes': int(held), 'peak_bytes': int(peak)}


run = {'label': args.label, 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
       'mha': measure(*MHA_SHAPE, expand=False), 'gqa': []}
print(json.dumps(run['mha']))
if not args.mha_only:
    for shape in GQA_SHAPES:
        N, H, KV, E, S = shape
        pair = [measure(*shape, expand=False), measure(*shape, expand=True)]
        saved = pair[1]['held_bytes'] - pair[0]['held_bytes']
        run['gqa'].append({'forms': pair, 'held_bytes_saved': saved,
                           'held_bytes_saved_expected': 2 * N * S * (H - KV) * E * 4})
        print(json.dumps(run['gqa'][-1]))
os.environ.pop('SPT_GQA_EXPAND', None)
out = {'runs': []}
if os.path.exists(args.out):
    with open(args.out) as f:
        out = json.load(f)
out['runs'].append(run)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
    f.write('\n')
