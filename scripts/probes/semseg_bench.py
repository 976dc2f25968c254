"""The semantic-segmentation step on one MI355X at the reference shape (resnet50_pfan_semantic_segmentation, 151 classes, 512 x 512,
bf16 autocast): the two kernels of csrc/semseg.hip against the same arithmetic in torch, and one full training step eager and
captured with the kernel-family breakdown of ops.KernelTimer.  Device-side timing (HIP events) for the kernels, a host clock around
synchronised windows for the steps; warm-up, several windows, median and spread.  Writes profiles/semseg_step.json -- the baseline
later changes are measured against; no threshold is attached to any number.

    python scripts/probes/semseg_bench.py [--batches 4 16 48] [--windows 5] [--steps 5] [--out profiles/semseg_step.json]

1. pixel_ce: ops.pixel_softmax_ce forward and backward in us and achieved bytes/s against rows*C*elem and 2*rows*C*elem; beside
   it the reference formula (float, permute, softmax, clamp, one-hot, log, multiply, sum, mean) in torch ops on the device.
2. cpfe: ops.cpfe_convs (one GEMM + tap gather) forward + backward against four torch convolutions + cat, at both CPFE inputs.
3. step: train_semantic_segmentation iterations, eager and with config.use_step_graph, per batch size; KernelTimer by family."""
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
import torch.nn.functional as F  # noqa: E402

from simpleaicv_pytorch_training_examples_amd import ops  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.SimpleAICV.semantic_segmentation import losses, models  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.tools import scripts, utils  # noqa: E402

PEAK_BYTES = 8.0e12
NUM_CLASSES, SIZE = 151, 512


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
    except RuntimeError as e:
        if 'exceeds 2^31 elements' not in str(e):
            raise
        return {'out_of_memory': str(e)}      # (the implicit-GEMM kernels index a tensor with 32 bits: the logits of 55 images do not fit)


def reference_ce(pred, label):
    """the reference CELoss formula in torch ops (semantic_segmentation/losses.py:22-43)"""
    pred = pred.float().permute(0, 2, 3, 1).contiguous()
    c = pred.shape[3]
    pred = torch.clamp(torch.softmax(pred, dim=-1), min=1e-4, max=1. - 1e-4).view(-1, c)
    onehot = F.one_hot(label.view(-1).long(), num_classes=c).float()
    return ((-torch.log(pred)) * onehot).sum(dim=-1).mean()


def bench_pixel_ce(batch, dtype, windows, steps):
    g = torch.Generator(device='cuda').manual_seed(0)
    logits = (torch.randn(batch, SIZE, SIZE, NUM_CLASSES, device='cuda', generator=g) * 3).to(dtype).permute(0, 3, 1, 2)
    label = torch.randint(0, NUM_CLASSES, (batch, SIZE, SIZE), device='cuda', generator=g).float()
    nbytes = logits.numel() * logits.element_size()
    res = {'batch': batch, 'dtype': str(dtype).replace('torch.', ''), 'rows': batch * SIZE * SIZE, 'classes': NUM_CLASSES,
           'logit_bytes': nbytes}
    x = logits.detach().requires_grad_(True)
    with torch.no_grad():
        res['kernel_forward'] = timed(lambda: ops.pixel_softmax_ce(logits, label), windows, steps)
    loss = ops.pixel_softmax_ce(x, label)
    res['kernel_backward'] = timed(lambda: torch.autograd.grad(loss, x, retain_graph=True), windows, steps)
    res['kernel_forward_bytes_per_s'] = nbytes / (res['kernel_forward']['median_us'] * 1e-6)
    res['kernel_backward_bytes_per_s'] = 2 * nbytes / (res['kernel_backward']['median_us'] * 1e-6)
    res['kernel_forward_fraction_of_hbm_peak'] = res['kernel_forward_bytes_per_s'] / PEAK_BYTES
    res['kernel_backward_fraction_of_hbm_peak'] = res['kernel_backward_bytes_per_s'] / PEAK_BYTES
    del loss

    def torch_side():
        out = {}
        with torch.no_grad():
            out['torch_forward'] = timed(lambda: reference_ce(logits, label), windows, steps)
        ref = reference_ce(x, label)
        out['torch_backward'] = timed(lambda: torch.autograd.grad(ref, x, retain_graph=True), windows, steps)
        out['loss_kernel_minus_torch'] = float(ops.pixel_softmax_ce(logits, label) - ref.detach())
        return out
    res.update(oom_safe(torch_side))
    if 'torch_forward' in res:
        res['torch_over_kernel_forward'] = res['torch_forward']['median_us'] / res['kernel_forward']['median_us']
        res['torch_over_kernel_backward'] = res['torch_backward']['median_us'] / res['kernel_backward']['median_us']
    return res


def bench_cpfe(batch, cin, hw, windows, steps):
    p, dil = 32, (3, 5, 7)
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(batch, hw, hw, cin, device='cuda', generator=g).permute(0, 3, 1, 2).requires_grad_(True)
    w1 = torch.nn.Parameter(torch.randn(p, cin, 1, 1, device='cuda', generator=g) / cin ** 0.5)
    wd = [torch.nn.Parameter(torch.randn(p, cin, 3, 3, device='cuda', generator=g) / (9 * cin) ** 0.5) for _ in dil]
    dout = torch.randn(batch, hw, hw, 4 * p, device='cuda', generator=g).permute(0, 3, 1, 2).bfloat16()

    def engine_side():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = ops.cpfe_convs(x, w1, wd, dil)
        torch.autograd.grad(out, [x, w1] + wd, dout)
        return out

    def torch_side():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = torch.cat([F.conv2d(x, w1)] + [F.conv2d(x, w, dilation=d, padding=d) for w, d in zip(wd, dil)], dim=1)
        torch.autograd.grad(out, [x, w1] + wd, dout)
        return out
    res = {'batch': batch, 'cin': cin, 'height_width': hw, 'planes': p,
           'gemm_flops_forward': 2.0 * batch * hw * hw * cin * 28 * p,
           'engine_forward_backward': timed(engine_side, windows, steps),
           'torch_forward_backward': timed(torch_side, windows, steps)}
    a, b = engine_side().float(), torch_side().float()
    res['output_rel_diff'] = float((a - b).abs().max() / b.abs().max())
    res['torch_over_engine'] = res['torch_forward_backward']['median_us'] / res['engine_forward_backward']['median_us']
    return res


def top_kernels(fn, k=14):
    """the k device kernels with the most time in one call of fn (torch.profiler): [name, launches, total us]"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.count, getattr(e, 'device_time_total', getattr(e, 'cuda_time_total', 0))) for e in prof.key_averages()]
        rows = sorted((r for r in rows if r[2] > 0), key=lambda r: -r[2])
        total = sum(r[2] for r in rows)
        return {'device_us_total': total, 'launches': sum(r[1] for r in rows), 'top': [[n[:96], c, round(t, 1)] for n, c, t in rows[:k]]}
    except Exception as e:      # the profiler is a convenience here, not the measurement
        return {'unavailable': str(e)}


class _Loader(list):
    dataset = ()


def bench_step(batch, windows, steps, use_graph, breakdown):
    class config:
        pass
    config.network = 'resnet50_pfan_semantic_segmentation'
    config.loss_ratio = {'CELoss': 1.0}
    config.optimizer = ('AdamW', {'lr': 1e-4, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    config.scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})
    config.epochs, config.batch_size, config.accumulation_steps, config.print_interval = 100, batch, 1, 10 ** 9
    config.use_amp, config.use_ema_model, config.local_rank, config.gpus_num, config.group = True, False, 0, 1, None
    config.sync_bn, config.host_sync_lag, config.use_step_graph, config.step_graph_warmup = False, 2, use_graph, 2
    torch.cuda.reset_peak_memory_stats()
    torch.manual_seed(0)
    model = models.__dict__[config.network](num_classes=NUM_CLASSES).cuda()
    criterion = {'CELoss': losses.CELoss()}
    optimizer, _ = utils.build_optimizer(config, model)
    scheduler = utils.Scheduler(config, optimizer)
    model, config.ema_model, config.scaler = utils.build_training_mode(config, model)
    g = torch.Generator().manual_seed(2)
    data = {'image': torch.randn(batch, SIZE, SIZE, 3, generator=g).permute(0, 3, 1, 2).cuda(),
            'mask': torch.randint(0, NUM_CLASSES, (batch, SIZE, SIZE), generator=g).float().cuda()}
    logger = logging.getLogger('semseg_bench')

    def epoch(n):
        loader = _Loader([data] * n)
        loader.dataset = [None] * (n * batch)
        return scripts.train_semantic_segmentation(loader, model, criterion, optimizer, scheduler, 1, logger, config)

    loss = epoch(4)                     # warm-up (and, with use_graph, the capture)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        loss = epoch(steps)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    res = {'batch': batch, 'captured': bool(use_graph), 'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms),
           'windows': windows, 'steps_per_window': steps, 'images_per_s': batch / (statistics.median(ms) * 1e-3), 'last_mean_loss': float(loss),
           'max_memory_gib': torch.cuda.max_memory_allocated() / 2 ** 30}
    if breakdown and not use_graph:
        timer = ops.KernelTimer
        timer.enabled, timer.only, timer.records = True, None, []
        epoch(2)
        torch.cuda.synchronize()
        summary = timer.summary()
        timer.enabled, timer.records = False, []
        res['kernel_families_ms_per_step'] = {k: {'ms': v['ms'] / 2, 'calls': v['calls'] // 2} for k, v in sorted(summary.items())}
        res['top_device_kernels'] = top_kernels(lambda: epoch(1))
        res['kernel_families_note'] = ('HIP-event brackets around the launches of each family in an eagerly launched step (host gaps '
                                       'between launches of a family count); families without a bracket (BatchNorm statistics of '
                                       'batch_norm2d, resize, activation, optimizer, torch ops) are the remainder')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[4, 16, 48], help='per-GPU batch sizes, the reference\'s 4 first; one that does not fit is reported as such')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'semseg_step.json'))
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('semseg_bench needs a GPU: nothing is measured without one')
    res = {'device': torch.cuda.get_device_name(), 'shape': f'{NUM_CLASSES} classes, {SIZE} x {SIZE}', 'pixel_ce': [], 'cpfe': [], 'step': []}
    for batch in args.batches:
        for dtype in (torch.bfloat16, torch.float32):
            res['pixel_ce'].append(oom_safe(lambda: bench_pixel_ce(batch, dtype, args.windows, args.steps * 4)))
            torch.cuda.empty_cache()
    for cin, hw in ((1024, SIZE // 16), (2048, SIZE // 32)):
        res['cpfe'].append(bench_cpfe(args.batches[0], cin, hw, args.windows, args.steps * 4))
    if not args.skip_step:
        for i, batch in enumerate(args.batches):
            for use_graph in (False, True):
                r = oom_safe(lambda: bench_step(batch, args.windows, args.steps, use_graph, breakdown=i == 0))
                r.setdefault('batch', batch)
                r.setdefault('captured', use_graph)
                res['step'].append(r)
                torch.cuda.empty_cache()
                if 'out_of_memory' in r:
                    break                       # a batch the eager step cannot hold is not captured either
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
