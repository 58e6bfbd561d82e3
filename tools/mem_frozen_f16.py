"""Peak memory and ms per step of an upgraded model with its frozen base weights in fp32 and in fp16
(`utils.store_frozen_fp16`), on the same box and build, one after the other.

    python tools/mem_frozen_f16.py --config llama-7b [--steps 8] [--warmup 3] [--layers N]
    python tools/mem_frozen_f16.py --config opt-1.3b

The model is built on the GPU with random weights rounded to the fp16 grid (what the upcast of a
checkpoint published in fp16 holds); a step is `SparseTuner.training_step` on synthetic tokens, as in
tools/bench_model.py.  The losses of both storages are printed side by side: they are the same numbers.
Prints one JSON object."""
import argparse, gc, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'spt-proto_amd'))
import torch
from naive_gpt import ext, models, utils

CONFIGS = {     # bench.py's: BASELINE.json configs[2], [3], [4]
    'bert-large': dict(family='opt', d_model=1024, n_heads=16, d_ff=4096, layers=24, vocab=30522, seq=512, batch=16),
    'opt-1.3b': dict(family='opt', d_model=2048, n_heads=32, d_ff=8192, layers=24, vocab=50272, seq=2048, batch=2),
    'llama-7b': dict(family='llama', d_model=4096, n_heads=32, d_ff=11008, layers=32, vocab=32000, seq=2048, batch=1),
}
ap = argparse.ArgumentParser()
ap.add_argument('--config', default='opt-1.3b', choices=sorted(CONFIGS))
ap.add_argument('--steps', type=int, default=8)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--layers', type=int, default=0, help='override the number of layers')
args = ap.parse_args()
c = dict(CONFIGS[args.config])
if args.layers:
    c['layers'] = args.layers
dev = 'cuda'


def build():
    torch.manual_seed(0)
    with torch.device(dev):           # (a 7B model is built on the GPU, not copied to it)
        model = (models.LLaMAModel if c['family'] == 'llama' else models.OPTModel)(
            d_model=c['d_model'], n_heads=c['n_heads'], n_layers=c['layers'], max_length=c['seq'],
            vocab_size=c['vocab'], d_feedforward=c['d_ff'], p_dropout=0.0)
        with torch.no_grad():
            for p in model.parameters():
                p.copy_(p.half().float())
        model = utils.upgrade_sparse(model, d_lora=16)
    return model.to(dev)


def run(stored):
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    ext.drop_images()
    ext.reset_paths()
    tuner = utils.SparseTuner(build(), frozen_fp16=stored)
    gen = torch.Generator(device=dev).manual_seed(1)
    losses = []

    def step():
        batch = torch.randint(3, c['vocab'], [c['batch'], c['seq'] + 2], device=dev, generator=gen)
        losses.append(tuner.training_step(batch))

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()      # (the build's own peak -- fp32 before the conversion -- aside)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    report = tuner.frozen_fp16_report
    res = {'ms_per_step': round(dt * 1e3, 3), 'peak_hbm_gb': round(torch.cuda.max_memory_allocated() / 1e9, 4),
           'resident_gb': round(resident / 1e9, 4), 'losses': [round(float(l), 6) for l in losses],
           'fallbacks': sorted('{}: {}'.format(*k) for k in ext.paths_taken() if k[1] in ('f16_upcast', 'torch_loop'))}
    if report is not None:
        res['converted_tensors'] = len(report['converted'])
        res['freed_gb'] = round(report['bytes_freed'] / 1e9, 4)
        res['kept'] = report['kept']
    tuner.release()
    del tuner
    return res


out = {'config': args.config, 'layers': c['layers'], 'seq': c['seq'], 'batch': c['batch'],
       'device': torch.cuda.get_device_name(0), 'fp32_storage': run(False), 'fp16_storage': run(True)}
a, b = out['fp32_storage'], out['fp16_storage']
out['peak_saved_gb'] = round(a['peak_hbm_gb'] - b['peak_hbm_gb'], 4)
out['step_time_ratio_fp16_over_fp32'] = round(b['ms_per_step'] / a['ms_per_step'], 4)
out['same_losses'] = a['losses'] == b['losses']
print(json.dumps(out, indent=1))
