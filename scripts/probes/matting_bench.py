"""The human-matting step on one MI355X at the reference shape (resnet50_pfan_matting, 1024 x 1024, bf16 autocast, the seven
losses of 07.human_matting_training): every fused loss of csrc/matting.hip against the reference formula as torch ops on the same
GPU (the losses' 'composed' route), forward + backward, and one full training step eager and captured with fused and with composed
losses.  Device-side timing (HIP events) for the losses, a host clock around synchronised windows for the steps; warm-up, several
windows, median and spread; the two routes alternate in one process.  Writes profiles/matting_step.json -- the baseline later
changes are measured against; no threshold is attached to any number.

    python scripts/probes/matting_bench.py [--batch 8] [--size 1024] [--windows 5] [--steps 5] [--out profiles/matting_step.json]

1. losses: per loss, fused and composed forward + backward in us; per kernel the forward alone, the backward by difference, and
   the achieved fraction of the HBM peak against the bytes per pixel the kernel has to move.
2. step: train_human_matting iterations, eager and with config.use_step_graph, fused and composed losses; KernelTimer by family."""
import argparse
import json
import logging
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from simpleaicv_pytorch_training_examples_amd import ops  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting import losses, models  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.tools import human_matting_scripts as scripts, utils  # noqa: E402

PEAK_BYTES = 8.0e12
NAMES = losses.__all__
# bytes per full-resolution pixel a kernel has to move: forward, backward (fp32 maps; the pyramid adds a third for its coarser levels:
# forward reads the level and writes a quarter of it, backward reads the level, a quarter of a gradient and writes the gradient)
BYTES = {'trimap_stats': (16, 28), 'alpha_l1_masked': (12, 16), 'alpha_l1': (8, 12), 'composition_l1': (40, 44),
         'laplacian_l1_masked': (12 + 4 * (1 / 4 + 5 / 16 * 4 / 3), 16 + 4 * (1 / 4 + 9 / 16 * 4 / 3)),
         'laplacian_l1': (8 + 4 * (1 / 4 + 5 / 16 * 4 / 3), 12 + 4 * (1 / 4 + 9 / 16 * 4 / 3)), 'matting_fuse': (20, 20)}


def timed(fn, windows, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / steps * 1e3)
    return {'median_us': statistics.median(us), 'min_us': min(us), 'max_us': max(us), 'windows': windows, 'steps_per_window': steps}


def safe(fn):
    try:
        return fn()
    except (torch.OutOfMemoryError, RuntimeError) as e:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return {'failed': str(e).splitlines()[0][:300]}


def make_batch(batch, size, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    d = {'image': torch.randn(batch, size, size, 3, device='cuda', generator=g).permute(0, 3, 1, 2),
         'mask': torch.rand(batch, size, size, device='cuda', generator=g) ** 2,
         'fg_map': torch.rand(batch, size, size, 3, device='cuda', generator=g).permute(0, 3, 1, 2).contiguous(),
         'bg_map': torch.rand(batch, size, size, 3, device='cuda', generator=g).permute(0, 3, 1, 2).contiguous()}
    blocks = torch.randint(0, 3, (batch, size // 32, size // 32), device='cuda', generator=g)
    d['trimap'] = torch.tensor([0., 128., 255.], device='cuda')[blocks].repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()
    return d


def bench_losses(batch, size, windows, steps):
    d = make_batch(batch, size)
    g = torch.Generator(device='cuda').manual_seed(1)
    gp = torch.sigmoid(4. * torch.randn(batch, 3, size, size, device='cuda', generator=g)).requires_grad_(True)
    local = torch.sigmoid(4. * torch.randn(batch, 1, size, size, device='cuda', generator=g)).requires_grad_(True)
    px = batch * size * size
    calls = {
        'GlobalTrimapCELoss': (lambda c: c(gp, d['trimap']), gp), 'GloabelTrimapIouLoss': (lambda c: c(gp, d['trimap']), gp),
        'LocalAlphaLoss': (lambda c: c(local, d['mask'], d['trimap']), local),
        'LocalLaplacianLoss': (lambda c: c(local, d['mask'], d['trimap']), local),
        'FusionAlphaLoss': (lambda c: c(local, d['mask']), local), 'FusionLaplacianLoss': (lambda c: c(local, d['mask']), local),
        'CompositionLoss': (lambda c: c(d['image'], d['mask'], d['fg_map'], d['bg_map'], local), local),
    }
    res = {'batch': batch, 'size': size, 'pixels': px, 'per_loss': {}, 'kernels': {}}
    for name in NAMES:
        call, leaf = calls[name]
        fused, composed = losses.__dict__[name](), losses.__dict__[name]()
        composed.route = 'composed'
        entry = {'rounds': []}
        for _ in range(2):                                   # alternate the two routes: the spread between rounds is the noise
            entry['rounds'].append({
                'fused_forward_backward': safe(lambda: timed(lambda: torch.autograd.grad(call(fused), leaf), windows, steps)),
                'composed_forward_backward': safe(lambda: timed(lambda: torch.autograd.grad(call(composed), leaf), windows, steps))})
        for k in ('fused_forward_backward', 'composed_forward_backward'):
            vals = [r[k]['median_us'] for r in entry['rounds'] if 'median_us' in r[k]]
            entry[k + '_median_us'] = statistics.median(vals) if vals else None
        if entry['fused_forward_backward_median_us'] and entry['composed_forward_backward_median_us']:
            entry['composed_over_fused'] = entry['composed_forward_backward_median_us'] / entry['fused_forward_backward_median_us']
        entry['value_fused_minus_composed'] = safe(lambda: float(call(fused).detach() - call(composed).detach()))
        res['per_loss'][name] = entry
        torch.cuda.empty_cache()
    # the kernels alone: forward under no_grad, backward = (forward + backward) - forward
    kernels = {
        'trimap_stats': (lambda: ops.trimap_stats(gp, d['trimap']).sum(), gp),
        'alpha_l1_masked': (lambda: ops.alpha_l1(local, d['mask'], d['trimap']).sum(), local),
        'alpha_l1': (lambda: ops.alpha_l1(local, d['mask']).sum(), local),
        'composition_l1': (lambda: ops.composition_l1(local, d['fg_map'], d['bg_map'], d['image']).sum(), local),
        'laplacian_l1_masked': (lambda: ops.laplacian_sums(local, d['mask'], d['trimap']).sum(), local),
        'laplacian_l1': (lambda: ops.laplacian_sums(local, d['mask']).sum(), local),
        'matting_fuse': (lambda: ops.collaborative_matting(gp, local).sum(), local),
    }
    for name, (fn, leaf) in kernels.items():
        def fwd():
            with torch.no_grad():
                return fn()
        f = timed(fwd, windows, steps)
        fb = timed(lambda: torch.autograd.grad(fn(), leaf), windows, steps)
        bwd_us = fb['median_us'] - f['median_us']
        res['kernels'][name] = {
            'forward': f, 'forward_backward': fb, 'backward_us_by_difference': bwd_us, 'bytes_per_pixel': BYTES[name],
            'forward_fraction_of_hbm_peak': BYTES[name][0] * px / (f['median_us'] * 1e-6) / PEAK_BYTES,
            'backward_fraction_of_hbm_peak': BYTES[name][1] * px / (bwd_us * 1e-6) / PEAK_BYTES if bwd_us > 0 else None,
            'note': 'includes the [B]-sized torch reduction of the result and, backward, its expand'}
    return res


class _Loader(list):
    dataset = ()


def bench_step(batch, size, windows, steps, use_graph, route, breakdown):
    class config:
        pass
    config.network = 'resnet50_pfan_matting'
    config.loss_ratio = {name: 1.0 for name in NAMES}
    config.optimizer = ('AdamW', {'lr': 1e-4, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    config.scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})
    config.epochs, config.batch_size, config.accumulation_steps, config.print_interval = 100, batch, 1, 10 ** 9
    config.use_amp, config.use_ema_model, config.local_rank, config.gpus_num, config.group = True, False, 0, 1, None
    config.sync_bn, config.host_sync_lag, config.use_step_graph, config.step_graph_warmup = False, 2, use_graph, 2
    torch.cuda.reset_peak_memory_stats()
    torch.manual_seed(0)
    model = models.__dict__[config.network]().cuda()
    criterion = {name: losses.__dict__[name]() for name in NAMES}
    for c in criterion.values():
        c.route = route
    optimizer, _ = utils.build_optimizer(config, model)
    scheduler = utils.Scheduler(config, optimizer)
    model, config.ema_model, config.scaler = utils.build_training_mode(config, model)
    data = make_batch(batch, size, seed=2)
    logger = logging.getLogger('matting_bench')

    def epoch(n):
        loader = _Loader([data] * n)
        loader.dataset = [None] * (n * batch)
        return scripts.train_human_matting(loader, model, criterion, optimizer, scheduler, 1, logger, config)

    loss = epoch(4)                     # warm-up (and, with use_graph, the capture)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        loss = epoch(steps)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    res = {'batch': batch, 'size': size, 'captured': bool(use_graph), 'loss_route': route, 'median_ms': statistics.median(ms),
           'min_ms': min(ms), 'max_ms': max(ms), 'windows': windows, 'steps_per_window': steps,
           'images_per_s': batch / (statistics.median(ms) * 1e-3), 'last_mean_loss': float(loss),
           'max_memory_gib': torch.cuda.max_memory_allocated() / 2 ** 30}
    if breakdown and not use_graph:
        timer = ops.KernelTimer
        timer.enabled, timer.only, timer.records = True, None, []
        epoch(2)
        torch.cuda.synchronize()
        summary = timer.summary()
        timer.enabled, timer.records = False, []
        res['kernel_families_ms_per_step'] = {k: {'ms': v['ms'] / 2, 'calls': v['calls'] // 2,
                                                  'fraction_of_hbm_peak': (v['bytes'] / PEAK_BYTES * 1e3 / v['ms']) if v['bytes'] and v['ms'] else None}
                                              for k, v in sorted(summary.items())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matting_step.json'))
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('matting_bench needs a GPU: nothing is measured without one')
    res = {'device': torch.cuda.get_device_name(), 'shape': f'batch {args.batch}, {args.size} x {args.size}, bf16 autocast'}
    res['losses'] = safe(lambda: bench_losses(args.batch, args.size, args.windows, args.steps * 2))
    torch.cuda.empty_cache()
    res['step'] = []
    if not args.skip_step:
        for use_graph, route in ((False, 'fused'), (False, 'composed'), (True, 'fused'), (True, 'composed')):
            r = safe(lambda: bench_step(args.batch, args.size, args.windows, args.steps, use_graph, route, breakdown=True))
            r.setdefault('captured', use_graph)
            r.setdefault('loss_route', route)
            res['step'].append(r)
            torch.cuda.empty_cache()
            if 'failed' in r and 'illegal' in r['failed'].lower():
                break                       # nothing more is started after a device fault
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
