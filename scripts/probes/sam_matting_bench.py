"""The SAM matting loss and step on one MI355X at the reference shape ([B, 4, ., 1024, 1024] predictions, fp32 as the model hands them
out): SAMMattingLoss forward + backward by three routes in one run --
  fused      ops.group_matting_stats + ops.group_laplacian_sums (csrc/matting.hip): targets read once per pixel for all four masks,
             the backward reads the selected mask only;
  composed   the reference formulas as torch ops on the device;
  expanded   the existing per-row kernels (ops.trimap_stats, alpha_l1, composition_l1, laplacian_sums) on targets repeated four times
             with repeat_interleave --
at the per-GPU batch of the reference config (48 on 8 GPUs: 6) and at batch 1, and one sam_b_matting training step split into
encoder, the five decoder + FUSION passes, loss and optimizer.  Device-side timing (HIP events), warm-up, several windows, median
and spread; the routes alternate in two rounds, and the spread between rounds and windows is the noise a difference is held against.
Writes profiles/sam_matting_step.json; it is a record, no test and not read by bench.py.

    python scripts/probes/sam_matting_bench.py [--batches 6 1] [--size 1024] [--windows 5] [--steps 20] [--skip-step]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from simpleaicv_pytorch_training_examples_amd import ops  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.SimpleAICV.interactive_segmentation import losses_matting as lm  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.SimpleAICV.interactive_segmentation.models.segment_anything_matting import \
    sam_matting  # noqa: E402

PEAK_BYTES = 8.0e12
MASKS = 4


def timed(fn, windows, steps, warmup=2):
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
    except torch.OutOfMemoryError as e:               # (any other error, a device fault among them, ends the probe: nothing more is started)
        torch.cuda.empty_cache()
        return {'failed': str(e).splitlines()[0][:300]}


def make_case(batch, size, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    d = {'image': torch.randn(batch, 3, size, size, device='cuda', generator=g),
         'mask': torch.rand(batch, 1, size, size, device='cuda', generator=g) ** 2,
         'fg_map': torch.rand(batch, 3, size, size, device='cuda', generator=g),
         'bg_map': torch.rand(batch, 3, size, size, device='cuda', generator=g)}
    blocks = torch.randint(0, 3, (batch, size // 32, size // 32), device='cuda', generator=g)
    d['trimap'] = torch.tensor([0., 128., 255.], device='cuda')[blocks].repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()
    d['global_preds'] = torch.sigmoid(4. * torch.randn(batch, MASKS, 3, size, size, device='cuda', generator=g)).requires_grad_(True)
    d['local_preds'] = torch.sigmoid(4. * torch.randn(batch, MASKS, 1, size, size, device='cuda', generator=g)).requires_grad_(True)
    d['fused_preds'] = torch.sigmoid(4. * torch.randn(batch, MASKS, 1, size, size, device='cuda', generator=g)).requires_grad_(True)
    d['iou_preds'] = torch.rand(batch, MASKS, device='cuda', generator=g).requires_grad_(True)
    return d


def expanded_tables(gp, lp, fp, iou, images, masks, trimaps, fg, bg, thr):
    """the eight tables from the per-row kernels on targets repeated M times (what the engine could do before the grouped kernels)"""
    b, m, _, h, w = gp.shape
    p = float(h * w)
    rep = lambda t: torch.repeat_interleave(t, m, dim=0)          # noqa: E731
    a, tm, im, f, g = rep(masks), rep(trimaps), rep(images), rep(fg), rep(bg)
    gp2, lp2, fp2 = gp.reshape(b * m, 3, h, w), lp.reshape(b * m, 1, h, w), fp.reshape(b * m, 1, h, w)
    ts = ops.trimap_stats(gp2, tm).view(b, m, 2)
    la = ops.alpha_l1(lp2, a, tm).view(b, m, 2)
    fa = ops.alpha_l1(fp2, a).view(b, m, 2)
    co = ops.composition_l1(fp2, f, g, im).view(b, m)
    inv = lm._lap_inverse_counts(gp.device, h, w)
    ll = (ops.laplacian_sums(lp2, a[:, 0], tm) * inv).sum(0).view(b, m)
    fl = (ops.laplacian_sums(fp2, a[:, 0]) * inv).sum(0).view(b, m)
    with torch.no_grad():
        pb, ab = torch.clamp(fp.squeeze(2), min=1e-4, max=1. - 1e-4) > thr, masks > thr
        gt = (pb & ab).flatten(2).sum(-1).float() / torch.clamp((pb | ab).flatten(2).sum(-1).float(), min=1e-6)
    ip = torch.nn.functional.mse_loss(iou.float(), torch.clamp(gt, min=0., max=1.), reduction='none')
    return [ts[..., 0] / (3. * p), ts[..., 1] / p, la[..., 0] / (la[..., 1].detach() + 1.), ll, fa[..., 0] / p, fl, co / (3. * p), ip]


class ExpandedLoss(lm.SAMMattingLoss):

    def tables(self, global_preds, local_preds, fused_preds, iou_preds, images, masks, trimaps, fg_maps, bg_maps):
        tabs = expanded_tables(global_preds, local_preds, fused_preds, iou_preds, images, masks, trimaps, fg_maps, bg_maps,
                               self.mask_threshold)
        return [t / global_preds.shape[0] for t in tabs]


def bench_loss(batch, size, windows, steps):
    d = make_case(batch, size)
    leaves = [d[k] for k in ('global_preds', 'local_preds', 'fused_preds', 'iou_preds')]
    targets = (d['mask'], d['trimap'], d['fg_map'], d['bg_map'])
    routes = {'fused': lm.SAMMattingLoss(route='fused'), 'composed': lm.SAMMattingLoss(route='composed'), 'expanded': ExpandedLoss()}

    def run(loss):
        out = loss(d['image'], [[t] for t in leaves], targets)
        return torch.autograd.grad(sum(out.values()), leaves)

    px = batch * size * size
    res = {'batch': batch, 'size': size, 'masks': MASKS, 'routes': {}, 'rounds': 2}
    for name in routes:
        res['routes'][name] = {'rounds': []}
    for _ in range(2):                                       # alternate the routes: the spread between rounds is part of the noise
        for name, loss in routes.items():
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            r = safe(lambda: timed(lambda: run(loss), windows, steps))
            r['peak_memory_gib'] = torch.cuda.max_memory_allocated() / 2 ** 30
            res['routes'][name]['rounds'].append(r)
    for name, entry in res['routes'].items():
        meds = [r['median_us'] for r in entry['rounds'] if 'median_us' in r]
        allw = [v for r in entry['rounds'] if 'median_us' in r for v in (r['min_us'], r['max_us'])]
        entry['median_us'] = statistics.median(meds) if meds else None
        entry['spread_us'] = (max(allw) - min(allw)) if allw else None
        entry['peak_memory_gib'] = max(r['peak_memory_gib'] for r in entry['rounds'])
    with torch.no_grad():
        vals = {n: {k: float(v) for k, v in routes[n](d['image'], [[t] for t in leaves], targets).items()} for n in routes}
    res['values'] = vals
    f, c = res['routes']['fused'], res['routes']['composed']
    if f['median_us'] and c['median_us']:
        res['composed_over_fused'] = c['median_us'] / f['median_us']
        res['fused_faster_beyond_spread'] = bool(c['median_us'] - f['median_us'] > max(f['spread_us'], c['spread_us']))
    # the new kernels alone: forward under no_grad, backward by difference, against the bytes they have to move (fp32 maps:
    # 11 target floats once, 5 prediction floats per mask forward; backward with one selected mask reads the targets and that
    # mask's 5 floats and writes all 5 M gradient floats)
    def stats():
        return ops.group_matting_stats(d['global_preds'], d['local_preds'], d['fused_preds'], d['mask'], d['trimap'], d['image'],
                                       d['fg_map'], d['bg_map'], 0.5)
    sel = torch.zeros(batch, MASKS, 8, device='cuda')
    sel[:, 1, :6] = 1.

    def fwd():
        with torch.no_grad():
            return stats()
    tf = timed(fwd, windows, steps)
    tb_sel = timed(lambda: torch.autograd.grad(stats(), leaves[:3], sel), windows, steps)
    tb_all = timed(lambda: torch.autograd.grad(stats(), leaves[:3], torch.ones_like(sel)), windows, steps)
    bytes_f = (44 + 20 * MASKS) * px
    bytes_b_sel, bytes_b_all = (44 + 20 + 20 * MASKS) * px, (44 + 40 * MASKS) * px
    res['group_matting_stats'] = {
        'forward': tf, 'forward_backward_one_mask': tb_sel, 'forward_backward_all_masks': tb_all,
        'forward_bytes': bytes_f, 'forward_fraction_of_hbm_peak': bytes_f / (tf['median_us'] * 1e-6) / PEAK_BYTES,
        'backward_one_mask_fraction_of_hbm_peak': bytes_b_sel / ((tb_sel['median_us'] - tf['median_us']) * 1e-6) / PEAK_BYTES,
        'backward_all_masks_fraction_of_hbm_peak': bytes_b_all / ((tb_all['median_us'] - tf['median_us']) * 1e-6) / PEAK_BYTES}
    lap_g = torch.zeros(6, batch * MASKS, device='cuda')
    lap_g[:, 1::MASKS] = 1.

    def lap():
        return ops.group_laplacian_sums(d['local_preds'], d['mask'], d['trimap'])

    def lap_fwd():
        with torch.no_grad():
            return lap()
    lf = timed(lap_fwd, windows, steps)
    lb_sel = timed(lambda: torch.autograd.grad(lap(), leaves[1], lap_g), windows, steps)
    lb_all = timed(lambda: torch.autograd.grad(lap(), leaves[1], torch.ones_like(lap_g)), windows, steps)
    lap_bytes_f = (4 * MASKS + 8) * px + 4 * MASKS * px * (1 / 4 + 5 / 16 * 4 / 3)
    # backward: level 0 reads the live rows' prediction, the targets and a quarter-size gradient and writes all M rows; the
    # coarser levels run for the live rows only (read the level and a quarter of a gradient, write the gradient)
    coarse_b = 4 * px * (1 / 4 + 9 / 16 * 4 / 3)
    lap_bytes_b_one = (4 + 8 + 4 * MASKS) * px + coarse_b
    lap_bytes_b_all = (4 * MASKS + 8 + 4 * MASKS) * px + MASKS * coarse_b
    res['group_laplacian_sums_masked'] = {
        'forward': lf, 'forward_backward_one_mask': lb_sel, 'forward_backward_all_masks': lb_all, 'forward_bytes': lap_bytes_f,
        'forward_fraction_of_hbm_peak': lap_bytes_f / (lf['median_us'] * 1e-6) / PEAK_BYTES,
        'backward_one_mask_us': lb_sel['median_us'] - lf['median_us'], 'backward_all_masks_us': lb_all['median_us'] - lf['median_us'],
        'backward_one_mask_fraction_of_hbm_peak': lap_bytes_b_one / ((lb_sel['median_us'] - lf['median_us']) * 1e-6) / PEAK_BYTES,
        'backward_all_masks_fraction_of_hbm_peak': lap_bytes_b_all / ((lb_all['median_us'] - lf['median_us']) * 1e-6) / PEAK_BYTES,
        'note': 'shares of the HBM peak are bytes the kernels have to move over event-time differences (forward + backward minus '
                'forward, windows of a few milliseconds), not a kernel trace: good to tens of per cent'}
    return res


def bench_step(batch, size, windows, steps, route):
    """one eager sam_b_matting step by parts, each a device-timed region: encoder forward, five decoder + FUSION passes forward,
    loss forward, the whole backward, AdamW"""
    torch.manual_seed(0)
    model = sam_matting.sam_b_matting(image_size=size).cuda().train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5, weight_decay=0.)
    loss = lm.SAMMattingLoss(route=route)
    d = make_case(batch, size, seed=3)
    box = torch.tensor([[size * 0.25, size * 0.25, size * 0.75, size * 0.75]] * batch, device='cuda')
    point = torch.tensor([[[size * 0.5, size * 0.5, 1.]]] * batch, device='cuda')
    targets = (d['mask'], d['trimap'], d['fg_map'], d['bg_map'])
    parts = {k: [] for k in ('encoder_forward', 'decoder_passes_forward', 'loss_forward', 'backward', 'optimizer', 'step')}

    def step(record):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        marks[0].record()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            emb = model.forward_image_encoder(d['image'])
        marks[1].record()
        outs_all = [[], [], [], []]
        prompts = {'prompt_point': point, 'prompt_box': box, 'prompt_mask': None}
        for i in range(5):
            with torch.autocast('cuda', dtype=torch.bfloat16):
                outs = model.forward_prompt_encoder_mask_decoder(emb, prompts)
            for acc, o in zip(outs_all, outs):
                acc.append(o)
            with torch.no_grad():
                best = outs[2][:, 0]
                prompts = {'prompt_point': point, 'prompt_box': box,
                           'prompt_mask': torch.nn.functional.interpolate(best, size=(size // 4, size // 4), mode='bilinear')}
        marks[2].record()
        value = sum(loss(d['image'], outs_all, targets).values())
        marks[3].record()
        value.backward()
        marks[4].record()
        opt.step()
        opt.zero_grad(set_to_none=True)
        marks[5].record()
        marks[5].synchronize()
        if record:
            for k, (a, b) in zip(list(parts)[:5], zip(marks[:-1], marks[1:])):
                parts[k].append(a.elapsed_time(b))
            parts['step'].append(marks[0].elapsed_time(marks[5]))

    torch.cuda.reset_peak_memory_stats()
    for _ in range(2):
        step(False)
    for _ in range(windows * steps):
        step(True)
    return {'batch': batch, 'size': size, 'loss_route': route, 'decoder_passes': 5, 'samples': windows * steps,
            'median_ms': {k: statistics.median(v) for k, v in parts.items()}, 'min_ms': {k: min(v) for k, v in parts.items()},
            'max_ms': {k: max(v) for k, v in parts.items()}, 'max_memory_gib': torch.cuda.max_memory_allocated() / 2 ** 30}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[6, 1])
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--step-batch', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sam_matting_step.json'))
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sam_matting_bench needs a GPU: nothing is measured without one')
    res = {'device': torch.cuda.get_device_name(), 'shape': f'[B, {MASKS}, ., {args.size}, {args.size}] fp32 predictions', 'loss': [],
           'step': []}
    for b in args.batches:
        r = safe(lambda: bench_loss(b, args.size, args.windows, args.steps))
        res['loss'].append(r)
        torch.cuda.empty_cache()
    ok = [r for r in res['loss'] if 'fused_faster_beyond_spread' in r]
    res['fused_is_default'] = bool(ok) and len(ok) == len(args.batches) and all(r['fused_faster_beyond_spread'] for r in ok)
    if not args.skip_step:
        for route in ('fused', 'composed'):
            r = safe(lambda: bench_step(args.step_batch, args.size, 2, 3, route))
            res['step'].append(r)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
