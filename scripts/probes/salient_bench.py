"""The salient-object-detection step on one MI355X at the reference shape (resnet50_pfan_segmentation, 1024 x 1024, bf16 autocast,
BCELoss + BCEIouloss): the two kernels of csrc/salient.hip against the same arithmetic in torch, and one full training step eager
and captured with the kernel-family breakdown of ops.KernelTimer.  Device-side timing (HIP events) for the kernels, a host clock
around synchronised windows for the steps; warm-up, several windows, median and spread.  Writes profiles/salient_step.json -- the
baseline later changes are measured against; no threshold is attached to any number.

    python scripts/probes/salient_bench.py [--batch 8] [--size 1024] [--windows 5] [--steps 5] [--out profiles/salient_step.json]

1. stats: ops.binary_seg_stats forward and backward in us and achieved bytes/s (8 and 12 bytes per element); beside it the
   reference's BCELoss + BCEIouloss + BCEDiceLoss formulas (float, permute, contiguous, clamp, log, multiply, sums) in torch ops.
2. head: ops.conv3x3_c1 forward + backward against ops.conv2d + torch.sigmoid on the same [batch, 32, size, size] bf16 activation,
   alternating in one process; achieved bytes/s of the fused kernel against 2 C + 4 bytes per pixel forward and 4 C + 8 backward.
3. step: train_salient_object_detection_segmentation iterations, eager and with config.use_step_graph (and eager with the generic
   head route); KernelTimer by family."""
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
from simpleaicv_pytorch_training_examples_amd.SimpleAICV.salient_object_detection import losses, models  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.tools import salient_object_detection_scripts as scripts, utils  # noqa: E402

PEAK_BYTES = 8.0e12
PLANES = 32


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


def oom_safe(fn):
    try:
        return fn()
    except torch.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {'out_of_memory': str(e).splitlines()[0]}


def reference_losses(pred, label):
    """BCELoss + BCEIouloss + BCEDiceLoss as the reference writes them (salient_object_detection/losses.py:16-134), torch ops"""
    total = 0.
    for kind in ('bce', 'iou', 'dice'):
        p = pred.float().permute(0, 2, 3, 1).contiguous()
        batch = p.shape[0]
        p = torch.clamp(p, min=1e-4, max=1. - 1e-4)
        if kind == 'bce':
            p, l = p.view(-1), label.view(-1)
            total = total + (-(l * torch.log(p) + (1. - l) * torch.log(1. - p))).mean()
            continue
        p, l = p.view(batch, -1), label.view(batch, -1)
        inter = p * l
        if kind == 'iou':
            total = total + (1. - (torch.sum(inter, dim=1) + 1e-4) / (torch.sum(p, dim=1) + torch.sum(l, dim=1) - torch.sum(inter, dim=1) + 1e-4)).mean()
        else:
            total = total + (1. - (2 * torch.sum(inter, dim=1) + 1e-4) / (torch.sum(p, dim=1) + torch.sum(l, dim=1) + 1e-4)).mean()
    return total


def bench_stats(batch, size, windows, steps):
    g = torch.Generator(device='cuda').manual_seed(0)
    pred = torch.sigmoid(6. * torch.randn(batch, 1, size, size, device='cuda', generator=g))
    label = torch.rand(batch, size, size, device='cuda', generator=g)
    n = pred.numel()
    crit = [losses.BCELoss(), losses.BCEIouloss(), losses.BCEDiceLoss()]
    res = {'batch': batch, 'size': size, 'elements': n}
    x = pred.detach().requires_grad_(True)

    def fused(p):
        p = p * 1.0 if p.requires_grad else p.view_as(p)           # a fresh tensor object: no result is reused between timed calls
        return sum(c(p, label) for c in crit)
    with torch.no_grad():
        res['kernel_forward'] = timed(lambda: fused(pred), windows, steps)
    res['kernel_forward_backward'] = timed(lambda: torch.autograd.grad(fused(x), x), windows, steps)
    with torch.no_grad():
        res['torch_forward'] = timed(lambda: reference_losses(pred, label), windows, steps)
    res['torch_forward_backward'] = timed(lambda: torch.autograd.grad(reference_losses(x, label), x), windows, steps)
    # the kernels alone (HIP events around the two launches, without the [B]-sized torch ops and the x * 1.0 copy)
    p2, l2 = pred.view(batch, -1), label.view(batch, -1)
    gstat = torch.randn(batch, 4, device='cuda')
    with torch.no_grad():
        res['stats_fwd_kernel'] = timed(lambda: ops.BinarySegStatsFn.apply(p2, l2), windows, steps)
    L = ops.lib()
    dp = torch.empty_like(p2)
    res['stats_bwd_kernel'] = timed(lambda: L.saicv_binary_seg_stats_bwd(p2.data_ptr(), l2.data_ptr(), gstat.data_ptr(), batch, p2.shape[1],
                                                                         dp.data_ptr(), ops.stream()), windows, steps)
    res['stats_fwd_fraction_of_hbm_peak'] = 8 * n / (res['stats_fwd_kernel']['median_us'] * 1e-6) / PEAK_BYTES
    res['stats_bwd_fraction_of_hbm_peak'] = 12 * n / (res['stats_bwd_kernel']['median_us'] * 1e-6) / PEAK_BYTES
    res['loss_kernel_minus_torch'] = float(fused(pred) - reference_losses(pred, label))
    res['torch_over_kernel_forward'] = res['torch_forward']['median_us'] / res['kernel_forward']['median_us']
    res['torch_over_kernel_forward_backward'] = res['torch_forward_backward']['median_us'] / res['kernel_forward_backward']['median_us']
    return res


def bench_head(batch, size, windows, steps):
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(batch, size, size, PLANES, device='cuda', generator=g).bfloat16().permute(0, 3, 1, 2).requires_grad_(True)
    conv = torch.nn.Conv2d(PLANES, 1, 3, padding=1).cuda()
    dout = torch.randn(batch, 1, size, size, device='cuda', generator=g)
    params = [x, conv.weight, conv.bias]

    def fused():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = ops.conv3x3_c1(x, conv.weight, conv.bias, sigmoid=True)
        torch.autograd.grad(out, params, dout)
        return out

    def generic():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = torch.sigmoid(ops.conv2d(x, conv.weight, conv.bias, 1, 1).float())
        torch.autograd.grad(out, params, dout)
        return out

    def fused_fwd():
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            return ops.conv3x3_c1(x, conv.weight, conv.bias, sigmoid=True)

    def generic_fwd():
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            return torch.sigmoid(ops.conv2d(x, conv.weight, conv.bias, 1, 1).float())
    px = batch * size * size
    res = {'batch': batch, 'size': size, 'planes': PLANES, 'pixels': px, 'rounds': []}
    for _ in range(2):                                  # alternate the two routes: the spread between rounds is the noise
        res['rounds'].append({'fused_forward_backward': timed(fused, windows, steps), 'generic_forward_backward': timed(generic, windows, steps),
                              'fused_forward': timed(fused_fwd, windows, steps), 'generic_forward': timed(generic_fwd, windows, steps)})
    for k in ('fused_forward_backward', 'generic_forward_backward', 'fused_forward', 'generic_forward'):
        res[k + '_median_us'] = statistics.median(r[k]['median_us'] for r in res['rounds'])
    fwd_bytes, bwd_bytes = px * (2 * PLANES + 4), px * (4 * PLANES + 8)
    res['fused_forward_fraction_of_hbm_peak'] = fwd_bytes / (res['fused_forward_median_us'] * 1e-6) / PEAK_BYTES
    bwd_us = res['fused_forward_backward_median_us'] - res['fused_forward_median_us']
    res['fused_backward_us_by_difference'] = bwd_us
    res['fused_backward_fraction_of_hbm_peak'] = bwd_bytes / (bwd_us * 1e-6) / PEAK_BYTES
    res['generic_over_fused_forward_backward'] = res['generic_forward_backward_median_us'] / res['fused_forward_backward_median_us']
    res['output_rel_diff'] = float((fused().float() - generic().float()).abs().max())
    return res


class _Loader(list):
    dataset = ()


def bench_step(batch, size, windows, steps, use_graph, head_route, breakdown):
    class config:
        pass
    config.network = 'resnet50_pfan_segmentation'
    config.loss_ratio = {'BCELoss': 1.0, 'BCEIouloss': 1.0}
    config.optimizer = ('AdamW', {'lr': 1e-4, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    config.scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})
    config.epochs, config.batch_size, config.accumulation_steps, config.print_interval = 100, batch, 1, 10 ** 9
    config.use_amp, config.use_ema_model, config.local_rank, config.gpus_num, config.group = True, False, 0, 1, None
    config.sync_bn, config.host_sync_lag, config.use_step_graph, config.step_graph_warmup = False, 2, use_graph, 2
    torch.cuda.reset_peak_memory_stats()
    torch.manual_seed(0)
    model = models.__dict__[config.network]().cuda()
    model.head_route = head_route
    criterion = {'BCELoss': losses.BCELoss(), 'BCEIouloss': losses.BCEIouloss()}
    optimizer, _ = utils.build_optimizer(config, model)
    scheduler = utils.Scheduler(config, optimizer)
    model, config.ema_model, config.scaler = utils.build_training_mode(config, model)
    g = torch.Generator().manual_seed(2)
    data = {'image': torch.randn(batch, size, size, 3, generator=g).permute(0, 3, 1, 2).cuda(),
            'mask': (torch.rand(batch, size, size, generator=g) ** 2).cuda()}
    logger = logging.getLogger('salient_bench')

    def epoch(n):
        loader = _Loader([data] * n)
        loader.dataset = [None] * (n * batch)
        return scripts.train_salient_object_detection_segmentation(loader, model, criterion, optimizer, scheduler, 1, logger, config)

    loss = epoch(4)                     # warm-up (and, with use_graph, the capture)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        loss = epoch(steps)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    res = {'batch': batch, 'size': size, 'captured': bool(use_graph), 'head_route': head_route, 'median_ms': statistics.median(ms),
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
        res['kernel_families_note'] = ('HIP-event brackets around the launches of each family in an eagerly launched step (host gaps '
                                       'between launches of a family count); fraction_of_hbm_peak = the family\'s algorithmic bytes '
                                       'over 8 TB/s over its bracketed time, for the families that report bytes')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'salient_step.json'))
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('salient_bench needs a GPU: nothing is measured without one')
    res = {'device': torch.cuda.get_device_name(), 'shape': f'batch {args.batch}, {args.size} x {args.size}, bf16 autocast'}
    res['stats'] = oom_safe(lambda: bench_stats(args.batch, args.size, args.windows, args.steps * 4))
    torch.cuda.empty_cache()
    res['head'] = oom_safe(lambda: bench_head(args.batch, args.size, args.windows, args.steps * 4))
    torch.cuda.empty_cache()
    res['step'] = []
    if not args.skip_step:
        for use_graph, route in ((False, 'fused'), (True, 'fused'), (False, 'generic')):
            r = oom_safe(lambda: bench_step(args.batch, args.size, args.windows, args.steps, use_graph, route, breakdown=True))
            r.setdefault('captured', use_graph)
            r.setdefault('head_route', route)
            res['step'].append(r)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
