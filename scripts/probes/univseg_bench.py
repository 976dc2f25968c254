"""The universal-segmentation set loss and step on one MI355X at the reference shape: mask_preds [16, 100, 512, 512] (batch 128 over
8 GPUs), bf16 as autocast hands them out and fp32, with T_i targets per image drawn from 1 .. 40 and at the worst case T_i = 150.

  loss   UniversalSegmentationLoss forward + backward by its two routes, alternating in two rounds (device events, warm-up,
         several windows, median and spread), peak memory of each, the fused route's kernels one by one against the bytes and the
         fp32 operations they have to move (share of the HBM peak and of the fp32 matrix peak; forward kernels under no_grad, the
         backward by difference), and the matcher's host side (the copy of the cost to the host plus scipy) on a host clock.
  step   one dinov3_vit_large_patch16_universal_segmentation step at batch 16, 512 x 512, bf16 autocast, split by device events into
         backbone, head + upsample, loss, backward and optimizer (Muon), and the x4 upsample with its backward timed alone.

Every block is stored with the shader clock rocm-smi reported while that block's work replayed after its timed windows.
Writes profiles/univseg_step.json; it is a record, no test and not read by bench.py.

    python scripts/probes/univseg_bench.py [--batch 16] [--size 512] [--windows 3] [--steps 3] [--skip-step] [--skip-loss]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

from bench import sample_power  # noqa: E402
from simpleaicv_pytorch_training_examples_amd import ops, ops_tfm  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation import models  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.segmentation_losses import \
    UniversalSegmentationLoss  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.tools.utils import build_optimizer  # noqa: E402

PEAK_BYTES = 8.0e12
PEAK_FP32 = 157.3e12
QUERIES, CLASSES = 100, 151


def timed(fn, windows, steps, warmup=1):
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


def clock(fn, seconds=1.0):
    got = sample_power(fn, torch.cuda.synchronize, seconds)
    return None if got is None else {'sclk_mhz': got['sclk_mhz'], 'socket_w': got['socket_w'], 'samples': got['samples']}


def make_case(batch, size, counts, dtype, seed=0):
    """block-structured binary targets of distinct classes per image, and logits that follow a target loosely for some queries"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    masks, labels = [], []
    for t in counts:
        cells = torch.randint(0, t, (size // 16, size // 16), device='cuda', generator=g)
        label_map = cells.repeat_interleave(16, 0).repeat_interleave(16, 1)
        masks.append(torch.stack([(label_map == k).float() for k in range(t)]))
        labels.append(torch.randperm(CLASSES - 1, device='cuda', generator=g)[:t])
    x = 4. * torch.randn(batch, QUERIES, size, size, device='cuda', generator=g)
    for b, t in enumerate(counts):
        x[b, :min(t, QUERIES)] += 3. * (2. * masks[b][:QUERIES] - 1.)
    cp = 2. * torch.randn(batch, QUERIES, CLASSES, device='cuda', generator=g)
    return x.to(dtype).requires_grad_(True), cp.requires_grad_(True), masks, labels


def bench_loss(batch, size, counts, dtype, windows, steps, tag):
    x, cp, masks, labels = make_case(batch, size, counts, dtype)
    crit = UniversalSegmentationLoss(num_classes=CLASSES).cuda()
    total, p = sum(counts), size * size
    es = x.element_size()

    def run(route):
        crit.route = route
        out = crit(x, cp, masks, labels)
        return torch.autograd.grad(sum(out.values()), [x, cp])

    res = {'case': tag, 'batch': batch, 'size': size, 'dtype': str(dtype), 'targets_per_image': counts, 'targets': total,
           'routes': {r: {'rounds': []} for r in ('fused', 'composed')}}
    for _ in range(2):                                       # alternate the routes: the spread between rounds is part of the noise
        for route in ('fused', 'composed'):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            r = timed(lambda: run(route), windows, steps)
            r['peak_memory_gib'] = torch.cuda.max_memory_allocated() / 2 ** 30
            res['routes'][route]['rounds'].append(r)
    for route, entry in res['routes'].items():
        entry['median_us'] = statistics.median(r['median_us'] for r in entry['rounds'])
        entry['spread_us'] = max(r['max_us'] for r in entry['rounds']) - min(r['min_us'] for r in entry['rounds'])
        entry['peak_memory_gib'] = max(r['peak_memory_gib'] for r in entry['rounds'])
        entry['clock'] = clock(lambda: run(route))
    f, c = res['routes']['fused'], res['routes']['composed']
    res['composed_over_fused'] = c['median_us'] / f['median_us']
    res['fused_faster_beyond_spread'] = bool(c['median_us'] - f['median_us'] > max(f['spread_us'], c['spread_us']))
    with torch.no_grad():
        vals = {}
        for route in ('fused', 'composed'):
            crit.route = route
            vals[route] = {k: float(v) for k, v in crit(x, cp, masks, labels).items()}
    res['values'] = vals

    # the fused route's pieces
    packed, off = torch.cat(masks), [0]
    for t in counts:
        off.append(off[-1] + t)
    lab = torch.cat(labels)
    xd = x.detach()
    pair = timed(lambda: ops.mask_pair_sums(xd, packed, off), windows, steps)
    pair_bytes, pair_flops = es * batch * QUERIES * p + 4 * total * p, 6.0 * QUERIES * total * p
    cost_t = timed(lambda: ops.mask_match_cost(xd, cp.detach(), packed, off, lab, 5., 5., 2.), windows, steps)
    torch.cuda.synchronize()
    host = []
    for _ in range(max(3, windows)):
        cost = ops.mask_match_cost(xd, cp.detach(), packed, off, lab, 5., 5., 2.)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c_host = cost.cpu()
        t1 = time.perf_counter()
        idx = [linear_sum_assignment(c_host[:, off[i]:off[i + 1]]) for i in range(batch)]
        host.append((t1 - t0, time.perf_counter() - t1))
    pb = torch.cat([torch.full((len(q), ), i, dtype=torch.int64) for i, (q, _) in enumerate(idx)])
    pq = torch.cat([torch.as_tensor(q, dtype=torch.int64) for q, _ in idx])
    pt = torch.cat([torch.as_tensor(t, dtype=torch.int64) + off[i] for i, (_, t) in enumerate(idx)])
    m = pb.numel()

    def stats():
        return ops.matched_mask_stats(x, packed, pb, pq, pt)

    def stats_fwd():
        with torch.no_grad():
            return stats()
    g = torch.rand(m, 4, device='cuda')
    sf = timed(stats_fwd, windows, steps)
    sb = timed(lambda: torch.autograd.grad(stats(), x, g), windows, steps)
    bwd_us = sb['median_us'] - sf['median_us']
    fwd_bytes, bwd_bytes = (es + 4) * m * p, es * batch * QUERIES * p + (es + 4) * m * p
    res['kernels'] = {
        'pair_sums': dict(pair, bytes=pair_bytes, flops=pair_flops,
                          fraction_of_hbm_peak=pair_bytes / (pair['median_us'] * 1e-6) / PEAK_BYTES,
                          fraction_of_fp32_matrix_peak=pair_flops / (pair['median_us'] * 1e-6) / PEAK_FP32,
                          bound='fp32 MFMA and the transcendentals, not HBM', clock=clock(lambda: ops.mask_pair_sums(xd, packed, off))),
        'match_cost_with_epilogue': cost_t,
        'matched_stats_forward': dict(sf, pairs=m, bytes=fwd_bytes, fraction_of_hbm_peak=fwd_bytes / (sf['median_us'] * 1e-6) / PEAK_BYTES),
        'matched_stats_backward': {'median_us': bwd_us, 'bytes': bwd_bytes, 'by': 'forward + backward minus forward',
                                   'forward_backward': sb, 'fraction_of_hbm_peak': bwd_bytes / (bwd_us * 1e-6) / PEAK_BYTES,
                                   'clock': clock(lambda: torch.autograd.grad(stats(), x, g))},
        'note': 'shares are the bytes / operations the kernels have to move over event-time windows, not a kernel trace',
    }
    res['matcher_host'] = {'copy_ms': statistics.median(h[0] for h in host) * 1e3, 'scipy_ms': statistics.median(h[1] for h in host) * 1e3,
                           'cost_bytes': 4 * QUERIES * total, 'samples': len(host), 'source': 'host clock after a device synchronise'}
    return res


def bench_step(batch, size, samples):
    """one eager dinov3_vit_large step by parts, each a device-timed region"""
    torch.manual_seed(0)
    model = models.dinov3_vit_large_patch16_universal_segmentation(image_size=size, query_num=QUERIES, num_classes=CLASSES).cuda().train()
    crit = UniversalSegmentationLoss(num_classes=CLASSES).cuda()
    cfg = type('Cfg', (), {'optimizer': ('Muon', {'lr': 4e-4, 'weight_decay': 1e-3, 'exclude_muon_layer_name_list': []})})
    opt, _ = build_optimizer(cfg, model)
    g = torch.Generator(device='cuda').manual_seed(5)
    counts = torch.randint(1, 41, (batch, ), generator=torch.Generator().manual_seed(5)).tolist()
    _, _, masks, labels = make_case(batch, size, counts, torch.bfloat16, seed=5)
    images = torch.randn(batch, 3, size, size, device='cuda', generator=g)
    parts = {k: [] for k in ('backbone_forward', 'head_upsample_forward', 'loss_forward', 'backward', 'optimizer', 'step')}
    net = model

    def step(record):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        marks[0].record()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            x = net.backbone.patch_embed(images)
            _, H, W, _ = x.shape
            x = x.flatten(1, 2)
            rope = net.backbone.rope_embed(H=H, W=W)
            for idx, block in enumerate(net.backbone.blocks):
                if idx == net.block_nums - net.query_block_nums:
                    x = torch.cat([net.query_embedding.weight[None].expand(batch, -1, -1).to(x.dtype), x], dim=1)
                x = block(x, rope)
            x = ops_tfm.layer_norm(x, net.backbone.norm.weight, net.backbone.norm.bias, net.backbone.norm.eps)
            marks[1].record()
            mask_preds, class_preds = net.predict(x)
            marks[2].record()
            value = sum(crit(mask_preds, class_preds, masks, labels).values())
        marks[3].record()
        value.backward()
        marks[4].record()
        opt.step()
        opt.zero_grad()
        marks[5].record()
        marks[5].synchronize()
        if record:
            for k, (a, b) in zip(list(parts)[:5], zip(marks[:-1], marks[1:])):
                parts[k].append(a.elapsed_time(b))
            parts['step'].append(marks[0].elapsed_time(marks[5]))

    res = {'batch': batch, 'size': size, 'model': 'dinov3_vit_large_patch16_universal_segmentation', 'autocast': 'bf16',
           'targets_per_image': counts, 'optimizer': 'engine.Muon through tools.utils.build_optimizer', 'routes': {}}
    for route in ('fused', 'composed'):
        crit.route = route
        for v in parts.values():
            v.clear()
        torch.cuda.reset_peak_memory_stats()
        step(False)
        for _ in range(samples):
            step(True)
        res['routes'][route] = {'samples': samples, 'median_ms': {k: statistics.median(v) for k, v in parts.items()},
                                'min_ms': {k: min(v) for k, v in parts.items()}, 'max_ms': {k: max(v) for k, v in parts.items()},
                                'max_memory_gib': torch.cuda.max_memory_allocated() / 2 ** 30, 'clock': clock(lambda: step(False), 2.0)}
    # the x4 upsample to [B, Q, size, size] and its backward alone (the follow-up would never form this tensor)
    low = torch.randn(batch, QUERIES, size // 4, size // 4, device='cuda', dtype=torch.bfloat16, requires_grad=True)
    gup = torch.randn(batch, QUERIES, size, size, device='cuda', dtype=torch.bfloat16)

    def up_fwd():
        with torch.no_grad():
            return ops_tfm.upsample4_bilinear(low)
    uf = timed(up_fwd, 3, 5)
    ub = timed(lambda: torch.autograd.grad(ops_tfm.upsample4_bilinear(low), low, gup), 3, 5)
    med = res['routes']['fused']['median_ms']
    res['upsample4'] = {'forward_us': uf['median_us'], 'forward_backward_us': ub['median_us'],
                        'share_of_fused_step': ub['median_us'] * 1e-3 / med['step'],
                        'loss_share_of_fused_step': med['loss_forward'] / med['step'],
                        'note': 'the loss backward is inside `backward`; the loss kernels read and write the [B, Q, size, size] tensor '
                                'the upsample forms'}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--step-samples', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'univseg_step.json'))
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--skip-loss', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('univseg_bench needs a GPU: nothing is measured without one')
    res = {'device': torch.cuda.get_device_name(), 'shape': f'[{args.batch}, {QUERIES}, {args.size}, {args.size}]', 'loss': [], 'step': None}
    drawn = torch.randint(1, 41, (args.batch, ), generator=torch.Generator().manual_seed(0)).tolist()
    if not args.skip_loss:
        for dtype in (torch.bfloat16, torch.float32):
            for tag, counts in (('T_i drawn from 1..40', drawn), ('worst case T_i = 150', [150] * args.batch)):
                res['loss'].append(bench_loss(args.batch, args.size, counts, dtype, args.windows, args.steps, tag))
                torch.cuda.empty_cache()
        ref = [r for r in res['loss'] if r['case'].startswith('T_i drawn')]
        res['fused_is_default'] = all(r['fused_faster_beyond_spread'] for r in ref)
    if not args.skip_step:
        res['step'] = bench_step(args.batch, args.size, args.step_samples)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
