"""Universal matting on one MI355X at the reference shape: predictions [8, 100, 3 | 1 | 1, 1024, 1024] fp32 in the channels-last
order the model's head writes (batch 32 over 4 accumulation steps), with 1 and with 4 objects per image.

  matcher  ops.matting_match_cost (csrc/unimat.hip) against the reference formulas as torch ops (matting_losses.composed_cost per
           image), alternating in two rounds; the pair-sum launch pair alone against the bytes it has to read (share of the HBM peak)
  head     ops.matting_head forward and forward + backward on bf16 logits against the torch expression (float, two sigmoids,
           collaborative_matting with torch.max), with its share of the HBM peak
  loss     UniversalMattingLoss forward + backward by its two routes
  step     one dinov3_vit_large_patch16_universal_matting step at batch 8, 1024 x 1024, bf16 autocast, Muon, split by device events
           into backbone, heads, loss, backward and optimizer

Device events, one warm-up, several windows, median and spread.  Writes profiles/unimat_step.json; it is a record, no test and not
read by bench.py.

    python scripts/probes/unimat_bench.py [--batch 8] [--size 1024] [--queries 100] [--windows 3] [--steps 10] [--skip-step]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from simpleaicv_pytorch_training_examples_amd import ops, ops_tfm  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation import matting_losses, models  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.tools.utils import build_optimizer  # noqa: E402

PEAK_BYTES = 8.0e12


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


def alternate(fns, windows, steps):
    """{name: fn} timed in two rounds, the routes alternating -> {name: {median_us, spread_us, rounds}}"""
    out = {k: {'rounds': []} for k in fns}
    for _ in range(2):
        for k, fn in fns.items():
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            r = timed(fn, windows, steps)
            r['peak_memory_gib'] = torch.cuda.max_memory_allocated() / 2 ** 30
            out[k]['rounds'].append(r)
    for entry in out.values():
        entry['median_us'] = statistics.median(r['median_us'] for r in entry['rounds'])
        entry['spread_us'] = max(r['max_us'] for r in entry['rounds']) - min(r['min_us'] for r in entry['rounds'])
        entry['peak_memory_gib'] = max(r['peak_memory_gib'] for r in entry['rounds'])
    return out


def make_targets(batch, size, per_image, g):
    alphas, trimaps, labels = [], [], []
    for _ in range(batch):
        coarse = torch.rand(per_image, size // 16, size // 16, device='cuda', generator=g)
        alpha = ((coarse.repeat_interleave(16, 1).repeat_interleave(16, 2) - 0.3) / 0.4).clamp(0, 1)
        alphas.append(alpha)
        trimaps.append(torch.where(alpha == 0, 0., torch.where(alpha == 1, 255., 128.)))
        labels.append(torch.zeros(per_image, dtype=torch.int64, device='cuda'))
    return trimaps, alphas, labels


def head_reference(gl, ll, q):
    """the reference's end of predict() as torch ops on NCHW-shaped logits"""
    b, _, h, w = gl.shape
    g = torch.sigmoid(gl.reshape(b, q, 3, h, w).float())
    l = torch.sigmoid(ll.reshape(b, q, 1, h, w).float())
    idx = torch.max(g, dim=2)[1].unsqueeze(2).float()
    tri = idx.clone()
    tri[tri == 2] = 0
    fg = idx.clone()
    fg[fg == 1] = 0
    fg[fg == 2] = 1
    return g, l, l * tri + fg


def bench_loss_side(batch, size, q, per_image, windows, steps):
    g = torch.Generator(device='cuda').manual_seed(per_image)
    p = size * size
    trimaps, alphas, labels = make_targets(batch, size, per_image, g)
    gl = (2 * torch.randn(batch, size, size, 3 * q, device='cuda', generator=g)).permute(0, 3, 1, 2)       # channels-last memory
    ll = (2 * torch.randn(batch, size, size, q, device='cuda', generator=g)).permute(0, 3, 1, 2)
    with torch.no_grad():
        gp, lp, fp = ops.matting_head(gl, ll)
    del gl, ll
    cp = torch.randn(batch, q, 2, device='cuda', generator=g)
    crit = matting_losses.UniversalMattingLoss(num_classes=2).cuda()
    off = [per_image * i for i in range(batch + 1)]
    tri, alp, lab = torch.cat(trimaps), torch.cat(alphas), torch.cat(labels)
    res = {'batch': batch, 'size': size, 'queries': q, 'objects_per_image': per_image}

    def composed_match():
        return crit.match_composed(gp, lp, fp, cp, trimaps, alphas, labels)

    def fused_match():
        return crit.match_fused(gp, lp, fp, cp, tri, alp, off, lab)

    assert all((a[0] == b[0]).all() and (a[1] == b[1]).all() for a, b in zip(fused_match(), composed_match()))
    res['matcher'] = alternate({'fused': fused_match, 'composed': composed_match}, windows, steps)
    pair = timed(lambda: ops.matting_pair_sums(gp, lp, fp, tri, alp, off), windows, steps)
    pair_bytes = 20 * batch * q * p + 8 * batch * per_image * p * ((q + 31) // 32)      # the targets are read once per query tile
    pair.update(bytes=pair_bytes, hbm_share=pair_bytes / PEAK_BYTES / (pair['median_us'] * 1e-6))
    res['pair_sums'] = pair

    leaves = [t.detach().requires_grad_(True) for t in (gp, lp, fp, cp)]

    def run(route):
        crit.route = route
        out = crit(*leaves, trimaps, alphas, labels)
        return torch.autograd.grad(sum(out.values()), leaves)

    res['loss_fwd_bwd'] = alternate({'fused': lambda: run('fused'), 'composed': lambda: run('composed')}, windows, steps)
    with torch.no_grad():
        vals = {}
        for route in ('fused', 'composed'):
            crit.route = route
            vals[route] = {k: float(v) for k, v in crit(*leaves, trimaps, alphas, labels).items()}
    res['values'] = vals
    for key in ('matcher', 'loss_fwd_bwd'):
        f, c = res[key]['fused'], res[key]['composed']
        res[key]['composed_over_fused'] = c['median_us'] / f['median_us']
        res[key]['fused_no_slower'] = bool(f['median_us'] <= c['median_us'] + max(f['spread_us'], c['spread_us']))
    return res


def bench_head(batch, size, q, windows, steps):
    g = torch.Generator(device='cuda').manual_seed(7)
    rows = batch * size * size
    gl = (2 * torch.randn(batch, size, size, 3 * q, device='cuda', generator=g)).bfloat16().permute(0, 3, 1, 2).requires_grad_(True)
    ll = (2 * torch.randn(batch, size, size, q, device='cuda', generator=g)).bfloat16().permute(0, 3, 1, 2).requires_grad_(True)

    def both(fn):
        outs = fn()
        torch.autograd.grad(outs, [gl, ll], [torch.ones_like(o) for o in outs])

    fused = lambda: ops.matting_head(gl, ll)                                   # noqa: E731
    torch_ops = lambda: head_reference(gl, ll, q)                              # noqa: E731
    with torch.no_grad():
        res = {'forward': alternate({'fused': fused, 'torch': torch_ops}, windows, steps)}
    res['forward_backward'] = alternate({'fused': lambda: both(fused), 'torch': lambda: both(torch_ops)}, windows, steps)
    fwd_bytes = rows * q * (4 * 2 + 5 * 4)
    bwd_bytes = rows * q * (4 * 4 + 5 * 4 + 4 * 2)
    f = res['forward']['fused']['median_us'] * 1e-6
    fb = res['forward_backward']['fused']['median_us'] * 1e-6
    res['hbm_share'] = {'forward': fwd_bytes / PEAK_BYTES / f, 'backward_by_difference': bwd_bytes / PEAK_BYTES / max(fb - f, 1e-9)}
    res['bytes'] = {'forward': fwd_bytes, 'backward': bwd_bytes}
    return res


def bench_step(batch, size, q, steps):
    torch.manual_seed(0)
    model = models.dinov3_universal_matting.dinov3_vit_large_patch16_universal_matting(image_size=size, query_num=q, num_classes=2).cuda().train()
    crit = matting_losses.UniversalMattingLoss(num_classes=2).cuda()

    class cfg:
        optimizer = ('Muon', {'lr': 4e-4, 'weight_decay': 1e-3, 'exclude_muon_layer_name_list': []})
    optimizer, _ = build_optimizer(cfg, model)
    g = torch.Generator(device='cuda').manual_seed(3)
    images = torch.randn(batch, 3, size, size, device='cuda', generator=g)
    trimaps, alphas, labels = make_targets(batch, size, 1, g)
    res = {}
    for route in ('fused', 'composed'):
        crit.route = route
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        parts = {k: [] for k in ('backbone', 'heads', 'loss', 'backward', 'optimizer', 'total')}
        for it in range(steps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record()
            with torch.autocast('cuda', dtype=torch.bfloat16):
                x = model.backbone.patch_embed(images)
                _, H, W, _ = x.shape
                x = x.flatten(1, 2)
                rope = model.backbone.rope_embed(H=H, W=W)
                for idx, block in enumerate(model.backbone.blocks):
                    if idx == model.block_nums - model.query_block_nums:
                        x = torch.cat([model.query_embedding.weight[None].expand(batch, -1, -1).to(x.dtype), x], dim=1)
                    x = block(x, rope)
                n = model.backbone.norm
                x = ops_tfm.layer_norm(x, n.weight, n.bias, n.eps)
                ev[1].record()
                outs = model.predict(x)
                ev[2].record()
                losses = crit(*outs, trimaps, alphas, labels)
            ev[3].record()
            sum(losses.values()).backward()
            ev[4].record()
            optimizer.step()
            optimizer.zero_grad()
            ev[5].record()
            ev[5].synchronize()
            if it:                                                       # the first iteration warms up
                for k, (a, b) in zip(parts, ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5))):
                    parts[k].append(ev[a].elapsed_time(ev[b]))
        res[route] = {k + '_ms': statistics.median(v) for k, v in parts.items()}
        res[route]['peak_memory_gib'] = torch.cuda.max_memory_allocated() / 2 ** 30
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--queries', type=int, default=100)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'unimat_step.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('unimat_bench measures on a GPU; none found')
    out = {'device': torch.cuda.get_device_name(0), 'hbm_peak_bytes_per_s': PEAK_BYTES, 'args': {k: v for k, v in vars(args).items() if k != 'out'}, 'loss': []}

    def save():
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)

    out['head'] = bench_head(args.batch, args.size, args.queries, args.windows, args.steps)
    print('head', json.dumps(out['head']['hbm_share']), flush=True)
    save()
    for per_image in (1, 4):
        out['loss'].append(bench_loss_side(args.batch, args.size, args.queries, per_image, args.windows, args.steps))
        r = out['loss'][-1]
        print(per_image, 'objects: matcher', {k: r['matcher'][k]['median_us'] for k in ('fused', 'composed')}, 'pair share',
              r['pair_sums']['hbm_share'], 'loss', {k: r['loss_fwd_bwd'][k]['median_us'] for k in ('fused', 'composed')}, flush=True)
        save()
    torch.cuda.empty_cache()
    if not args.skip_step:
        out['step'] = bench_step(args.batch, args.size, args.queries, args.steps)
        print('step', json.dumps(out['step']), flush=True)
        save()


if __name__ == '__main__':
    main()
