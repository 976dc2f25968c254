"""Records tests/golden/pfan_mat_r18_tiny.pt by RUNNING THE REFERENCE implementation on the CPU in fp32.  The fixture holds recorded
tensors, names and settings only; every input is regenerated from a seed by the recipes of tests/matting_common.py.

  model   resnet18_pfan_matting (SimpleAICV/human_matting/models/pfan_matting.py) built under torch.manual_seed(0), train mode, a
          seeded batch of 2 x 3 x 64 x 96 with alpha, trimap, fg and bg: config, input_shape, keys (sorted state_dict names with
          shapes), init_sample (16 points of every initial floating tensor), out (global, local, fused), losses (the seven
          losses of those outputs), grad_norm / grad_sample of every parameter and bn_buffers for the sum of the FOUR ARGMAX-FREE
          losses (both trimap losses, both local losses: a pixel whose two largest global probabilities nearly tie may take the
          other branch of collaborative_matting on other arithmetic, so the fused losses are judged on recorded outputs only),
          bf16_dev (how far the reference's own bf16-autocast global / local outputs move), tie_share (pixels whose two largest
          global probabilities are closer than 2e-3), grad_norm64 / bn_absmax64 (the same step in float64: which gradients and
          running means are exactly zero).  In the float64 step LocalLaplacianLoss is the reference formula as
          tests/matting_common.py writes it (the reference class builds an fp32 filter that a float64 convolution refuses).
  gauss   the 25 weights of LocalLaplacianLoss.build_gauss_kernel(size=5, sigma=1.0)
  losses  loss_cases: {(B, H, W): {loss name: value}} -- the reference losses at the kernel-test shapes (the two Laplacian losses
          where both sides reach 32); lap_dev: {(B, H, W, masked): {'loss', 'grad'}} -- how far the reference's own fp32
          Laplacian loss and its gradient lie from the float64 judge (relative to the loss / to the largest gradient element)
  eval    the reference EvalMeter (tools/human_matting_scripts.py:26-171) on two seeded batches with thresh [0.2, 0.5]

    python scripts/record_pfan_matting_golden.py --reference /path/to/reference/checkout

The reference packages import cv2 / torchvision / pycocotools / tqdm / thop / calflops at module scope for dataset and profiling
code; empty stand-ins are registered first.  EvalMeter.cal_conn calls cv2.connectedComponentsWithStats(intersection,
connectivity=4) and reads the label map and the last column of the statistics (the areas, background first): for that one call
the cv2 stand-in carries a function over scipy.ndimage.label with the 4-connected structure, labels numbered in scan order as
OpenCV numbers them.  No test imports this script."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'pfan_mat_r18_tiny.pt')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import matting_common as M  # noqa: E402

CONFIG = dict()
BATCH, H, W = 2, 64, 96


def sample_idx(numel, k=16):
    return torch.linspace(0, numel - 1, min(k, numel)).long()


class _Stub(types.ModuleType):
    """a module whose every attribute is another stub (the reference's dataset / profiling imports are never called here)"""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return _Stub(self.__name__ + '.' + name)

    def __call__(self, *a, **k):
        return None


def connected_components_with_stats(image, connectivity=4):
    from scipy import ndimage
    assert connectivity == 4
    labels, n = ndimage.label(image, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    areas = np.bincount(labels.reshape(-1), minlength=n + 1)
    stats = np.zeros((n + 1, 5), dtype=np.int32)
    stats[:, -1] = areas
    return n + 1, labels, stats, None


def call_loss(ref_losses, name, outs, x, alpha, trimap, fg, bg):
    g, l, f = outs
    fn = ref_losses.__dict__[name]()
    if name in ('GlobalTrimapCELoss', 'GloabelTrimapIouLoss'):
        return fn(g, trimap)
    if name in ('LocalAlphaLoss', 'LocalLaplacianLoss'):
        return fn(l, alpha, trimap)
    if name in ('FusionAlphaLoss', 'FusionLaplacianLoss'):
        return fn(f, alpha)
    return fn(x, alpha, fg, bg, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference implementation')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    for name in ['cv2', 'torchvision', 'torchvision.ops', 'torchvision.transforms', 'pycocotools', 'pycocotools.mask',
                 'pycocotools.cocoeval', 'pycocotools.coco', 'tqdm', 'thop', 'calflops', 'apex', 'yapf', 'yapf.yapflib',
                 'yapf.yapflib.yapf_api']:
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
    sys.modules['tqdm'].tqdm = lambda it, *a, **k: it
    sys.modules['cv2'].connectedComponentsWithStats = connected_components_with_stats
    from SimpleAICV.human_matting.models import pfan_matting as ref_models
    from SimpleAICV.human_matting import losses as ref_losses
    from tools.human_matting_scripts import EvalMeter

    x, alpha, trimap, fg, bg = M.model_inputs((BATCH, 3, H, W))

    model = None
    torch.manual_seed(0)
    model = ref_models.resnet18_pfan_matting(**CONFIG)
    model.train()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    outs = model(x)
    assert all(o.dtype == torch.float32 for o in outs) and tuple(outs[0].shape) == (BATCH, 3, H, W)
    detached = tuple(o.detach() for o in outs)
    losses = {name: float(call_loss(ref_losses, name, detached, x, alpha, trimap, fg, bg)) for name in M.LOSS_NAMES}
    sum(call_loss(ref_losses, name, outs, x, alpha, trimap, fg, bg) for name in M.ARGMAX_FREE).backward()
    top2 = torch.sort(detached[0], dim=1, descending=True)[0]
    fx = {
        'config': CONFIG, 'input_shape': (BATCH, 3, H, W),
        'keys': [(k, tuple(v.shape)) for k, v in sorted(init.items())],
        'init_sample': {k: v.flatten()[sample_idx(v.numel())].clone() for k, v in init.items() if v.dtype.is_floating_point},
        'out': tuple(o.clone() for o in detached), 'losses': losses,
        'grad_norm': {k: float(p.grad.norm()) for k, p in model.named_parameters() if p.grad is not None},
        'grad_sample': {k: p.grad.flatten()[sample_idx(p.numel())].clone() for k, p in model.named_parameters() if p.grad is not None},
        'bn_buffers': {k: v.clone() for k, v in model.state_dict().items() if 'running_' in k},
        'tie_share': float(((top2[:, 0] - top2[:, 1]) < 2e-3).float().mean()),
        'gauss': ref_losses.LocalLaplacianLoss().build_gauss_kernel(size=5, sigma=1.0, n_channels=1).reshape(25).clone(),
    }
    torch.manual_seed(0)
    model2 = ref_models.resnet18_pfan_matting(**CONFIG)
    model2.train()
    with torch.autocast('cpu', dtype=torch.bfloat16):
        outs2 = model2(x)
    fx['bf16_dev'] = max(float((a.float() - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(outs2[:2], detached[:2]))

    # float64 arbiter of the four argmax-free losses (the reference's .float() calls would round it to fp32)
    torch.manual_seed(0)
    model3 = ref_models.resnet18_pfan_matting(**CONFIG).double()
    model3.train()
    float_orig = torch.Tensor.float
    torch.Tensor.float = lambda self: self if self.dtype == torch.float64 else float_orig(self)
    try:
        outs3 = model3(x.double())
        assert outs3[0].dtype == torch.float64
        a64, t64 = alpha.double(), trimap.double()
        (ref_losses.GlobalTrimapCELoss()(outs3[0], t64) + ref_losses.GloabelTrimapIouLoss()(outs3[0], t64)
         + ref_losses.LocalAlphaLoss()(outs3[1], a64, t64) + M.lap_loss_reference_form(outs3[1], a64, t64)).backward()
    finally:
        torch.Tensor.float = float_orig
    fx['grad_norm64'] = {k: float(p.grad.norm()) for k, p in model3.named_parameters() if p.grad is not None}
    fx['bn_absmax64'] = {k: float(v.abs().max()) for k, v in model3.state_dict().items() if 'running_' in k}
    print('exactly-zero statistics:', [k for k, v in fx['bn_buffers'].items() if fx['bn_absmax64'][k] < 1e-3 * float(v.abs().max())])
    print('exactly-zero gradients:', [k for k, n in fx['grad_norm'].items() if fx['grad_norm64'][k] < 1e-3 * n])

    fx['loss_cases'] = {}
    for case in M.PIXEL_CASES:
        d = M.pixel_inputs(*case)
        fused, _ = M.fuse_judge(d['global_pred'], d['local_pred'])
        names = [n for n in M.LOSS_NAMES if 'Laplacian' not in n or min(case[1:]) >= 32]
        fx['loss_cases'][case] = {n: float(call_loss(ref_losses, n, (d['global_pred'], d['local_pred'], fused), d['image'], d['alpha'],
                                                     d['trimap'], d['fg'], d['bg'])) for n in names}
    fx['lap_dev'] = {}
    for case in M.LAP_CASES:
        for masked in (False, True):
            pred, al, tm = M.lap_float_inputs(*case, masked)
            loss64, grad64, _ = M.lap_loss_judge(pred, al, tm)
            leaf = pred.clone().requires_grad_(True)
            loss = ref_losses.LocalLaplacianLoss()(leaf, al, tm) if masked else ref_losses.FusionLaplacianLoss()(leaf, al)
            loss.backward()
            fx['lap_dev'][case + (masked,)] = {'loss': abs(float(loss) - float(loss64)) / abs(float(loss64)),
                                               'grad': float((leaf.grad.double() - grad64).abs().max() / grad64.abs().max())}
    print('reference fp32 Laplacian losses against the float64 judge:', fx['lap_dev'])

    class cfg:
        thresh, squared_beta = M.EVAL_THRESH, M.EVAL_SQUARED_BETA
    meter = EvalMeter(cfg)
    for preds, masks in M.eval_inputs():
        meter.add_batch_result(preds, masks)
    meter.compute_all_metrics()
    fx['eval'] = {k: (np.asarray(getattr(meter, k)).tolist()) for k in M.EVAL_KEYS}
    torch.save(fx, OUT)
    print('out', [tuple(o.shape) for o in detached], 'losses', losses, 'params with gradient', len(fx['grad_norm']), 'bf16 deviation',
          fx['bf16_dev'], 'tie share', fx['tie_share'], 'eval', fx['eval'], 'bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
