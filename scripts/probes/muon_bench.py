"""engine.Muon.step() on ViT-B/16 against the same algorithm written with torch bf16 matmuls (the reference's method without its
compiler), same GPU, same process.  The gradient arena is filled once; both sides step their own copy of the parameters.
Device-side timing (HIP events), warm-up, several windows; median and spread.  Writes profiles/muon_step.json.

    python scripts/probes/muon_bench.py [--windows 7] [--steps 10] [--out profiles/muon_step.json] [--only-engine]

--only-engine runs nothing but warm-up + timed engine steps: the form to put under `rocprofv3 --kernel-trace --stats` for the
launch count and the per-kernel times."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from simpleaicv_pytorch_training_examples_amd import engine  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification import backbones  # noqa: E402
from simpleaicv_pytorch_training_examples_amd.tools import utils  # noqa: E402

PEAK_TFLOPS = 2500.0
COEFFS = (3.4445, -4.7750, 2.0315)


def torch_newton_schulz(g, steps):
    a, b, c = COEFFS
    x = g.to(torch.bfloat16)
    tr = x.size(0) > x.size(1)
    if tr:
        x = x.mT
    x = x / (x.norm() + 1e-7)
    for _ in range(steps):
        aa = x @ x.mT
        bb = b * aa + c * aa @ aa
        x = a * x + bb @ x
    return x.mT if tr else x


class TorchMuon:
    """The reference's update rules, one parameter at a time, eager torch."""

    def __init__(self, muon, adamw, lr, wd, momentum=0.95, ns_steps=5, betas=(0.9, 0.999), eps=1e-8):
        self.muon, self.adamw, self.lr, self.wd, self.momentum, self.ns_steps, self.betas, self.eps = \
            muon, adamw, lr, wd, momentum, ns_steps, betas, eps
        self.buf = [torch.zeros_like(g.reshape(g.size(0), -1)) for _, g in muon]
        self.m1 = [torch.zeros_like(g) for _, g in adamw]
        self.m2 = [torch.zeros_like(g) for _, g in adamw]
        self.t = 0

    @torch.no_grad()
    def step(self):
        for (p, g), buf in zip(self.muon, self.buf):
            g2 = g.reshape(g.size(0), -1)
            buf.mul_(self.momentum).add_(g2)
            u = torch_newton_schulz(g2.add(buf, alpha=self.momentum), self.ns_steps)
            p.mul_(1 - self.lr * self.wd)
            p.add_(u.reshape(p.shape), alpha=-self.lr * 0.2 * math.sqrt(max(p.shape[0], p.shape[1])))
        self.t += 1
        b1, b2 = self.betas
        scale = (1 - b1 ** self.t) / (1 - b2 ** self.t) ** 0.5
        for (p, g), m1, m2 in zip(self.adamw, self.m1, self.m2):
            m1.lerp_(g, 1 - b1)
            m2.lerp_(g.square(), 1 - b2)
            p.mul_(1 - self.lr * self.wd)
            p.add_(m1 / (self.eps + m2.sqrt()), alpha=-self.lr / scale)


def timed(fn, windows, steps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'windows': windows, 'steps_per_window': steps}


def launches_of(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if getattr(e, 'device_time_total', getattr(e, 'cuda_time_total', 0)) > 0)
    except Exception as e:      # the profiler is a convenience here, not the measurement
        print(f'[muon_bench] no launch count from torch.profiler: {e}')
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'muon_step.json'))
    ap.add_argument('--only-engine', action='store_true')
    args = ap.parse_args()

    torch.manual_seed(0)
    model = backbones.vit_base_patch16(num_classes=1000).cuda()

    class config:
        optimizer = ('Muon', {'lr': 4e-4, 'weight_decay': 1e-3})
    opt, summary = utils.build_optimizer(config, model)
    assert isinstance(opt, engine.Muon)
    arena = opt.arena
    arena.flat_grad.normal_(generator=torch.Generator(device='cuda').manual_seed(1))
    arena.arrived = [True] * len(arena.params)
    plan = opt.plan
    ns_steps = opt.param_groups[0]['ns_steps']
    # useful work of the three stages (dense formulas) and the work the kernels really do (padded tiles, half of A and B)
    useful = sum(ns_steps * (4 * m * m * n + 2 * m ** 3) for _, _, _, m, n, _ in plan.items)
    done = ns_steps * sum((mp // 64) * (mp // 64 + 1) // 2 * 64 * 64 * 2 * (np_ + mp) + mp * np_ * 2 * mp for _, mp, np_, _, _, _ in plan.items)

    if args.only_engine:
        print(json.dumps({'engine_step': timed(opt.step, args.windows, args.steps)}))
        return

    named = dict(model.named_parameters())
    muon = [(named[n].detach().clone(), named[n].grad.detach().clone()) for n in summary[0]['name']]
    adamw = [(named[n].detach().clone(), named[n].grad.detach().clone()) for n in summary[1]['name']]
    ref = TorchMuon(muon, adamw, lr=4e-4, wd=1e-3)

    res = {
        'model': 'vit_base_patch16', 'muon_matrices': plan.nprob, 'backup_parameters': len(adamw), 'ns_steps': ns_steps,
        'engine_step': timed(opt.step, args.windows, args.steps),
        'engine_newton_schulz_only': timed(lambda: plan.run(ns_steps), args.windows, args.steps),
        'torch_bf16_step': timed(ref.step, args.windows, args.steps),
        'engine_launches_per_step': launches_of(opt.step), 'engine_launches_by_construction': 4 + 3 * ns_steps,
        'torch_launches_per_step': launches_of(ref.step),
        'useful_tflop_per_step': useful / 1e12, 'computed_tflop_per_step': done / 1e12,
    }
    ns_ms = res['engine_newton_schulz_only']['median_ms']
    res['stages_useful_tflops'] = useful / 1e9 / ns_ms
    res['stages_computed_tflops'] = done / 1e9 / ns_ms
    res['stages_fraction_of_peak'] = res['stages_computed_tflops'] / PEAK_TFLOPS
    res['torch_over_engine'] = res['torch_bf16_step']['median_ms'] / res['engine_step']['median_ms']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
