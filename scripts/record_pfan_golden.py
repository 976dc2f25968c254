"""Records tests/golden/pfan_r18_tiny.pt by RUNNING THE REFERENCE implementation on the CPU in fp32:
resnet18_pfan_semantic_segmentation(num_classes=7) (SimpleAICV/semantic_segmentation/models/pfan_semantic_segmentation.py) built
under torch.manual_seed(0), in train mode, on a seeded batch of 2 x 3 x 64 x 96, the reference CELoss (losses.py:13-43) on a seeded
integer mask, and one backward.  The fixture holds recorded tensors, names and settings only:

  config, input_shape, keys (sorted state_dict names with shapes), init_sample (16 points of every initial floating tensor),
  out (the prediction), loss, grad_norm / grad_sample (every parameter), bn_buffers (running statistics after the step),
  bf16_dev (how far the reference's own bf16-autocast output moves from its fp32 output),
  grad_norm64 (the gradient norms of the same model run in float64: a BatchNorm bias whose only consumer is a pointwise
  convolution followed by another batch-statistics BatchNorm has an exactly zero gradient -- the fp32 numbers of such a tensor are
  rounding noise, and the float64 norm, ten orders of magnitude smaller, says so), bn_absmax64 (the largest magnitude of every
  running statistic in that float64 run: the running mean behind two zero-mean inputs and a pointwise convolution is exactly zero too).

    python scripts/record_pfan_golden.py --reference /path/to/reference/checkout

The reference packages import cv2 / torchvision / pycocotools / tqdm / thop / calflops at module scope for dataset and
profiling code; empty stand-ins are registered first.  No test imports this script; the product-side tests rebuild the same model
under the same seed and compare."""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'pfan_r18_tiny.pt')

CONFIG = dict(num_classes=7)
BATCH, H, W = 2, 64, 96


def sample_idx(numel, k=16):
    return torch.linspace(0, numel - 1, min(k, numel)).long()


def inputs():
    x = torch.randn(BATCH, H, W, 3, generator=torch.Generator().manual_seed(1)).permute(0, 3, 1, 2)      # NHWC memory
    mask = torch.randint(0, CONFIG['num_classes'], (BATCH, H, W), generator=torch.Generator().manual_seed(2)).float()
    return x, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference implementation')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    for name in ['cv2', 'torchvision', 'torchvision.ops', 'torchvision.transforms', 'pycocotools', 'pycocotools.mask',
                 'pycocotools.cocoeval', 'pycocotools.coco', 'tqdm', 'thop', 'calflops']:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['tqdm'].tqdm = lambda it, *a, **k: it
    from SimpleAICV.semantic_segmentation.models import pfan_semantic_segmentation as ref_models
    from SimpleAICV.semantic_segmentation.losses import CELoss

    torch.manual_seed(0)
    model = ref_models.resnet18_pfan_semantic_segmentation(**CONFIG)
    model.train()
    x, mask = inputs()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    out = model(x)
    loss = CELoss()(out, mask)
    loss.backward()
    fx = {
        'config': CONFIG, 'input_shape': (BATCH, 3, H, W),
        'keys': [(k, tuple(v.shape)) for k, v in sorted(init.items())],
        'init_sample': {k: v.flatten()[sample_idx(v.numel())].clone() for k, v in init.items() if v.dtype.is_floating_point},
        'out': out.detach().clone(), 'loss': float(loss.detach()),
        'grad_norm': {k: float(p.grad.norm()) for k, p in model.named_parameters() if p.grad is not None},
        'grad_sample': {k: p.grad.flatten()[sample_idx(p.numel())].clone() for k, p in model.named_parameters() if p.grad is not None},
        'bn_buffers': {k: v.clone() for k, v in model.state_dict().items() if 'running_' in k},
    }
    torch.manual_seed(0)
    model2 = ref_models.resnet18_pfan_semantic_segmentation(**CONFIG)
    model2.train()
    with torch.autocast('cpu', dtype=torch.bfloat16):
        out2 = model2(x)
    fx['bf16_dev'] = float((out2.float() - out.detach()).abs().max() / out.detach().abs().max().clamp_min(1e-30))
    torch.manual_seed(0)
    model3 = ref_models.resnet18_pfan_semantic_segmentation(**CONFIG).double()
    model3.train()
    CELoss()(model3(x.double()), mask).backward()
    fx['grad_norm64'] = {k: float(p.grad.norm()) for k, p in model3.named_parameters() if p.grad is not None}
    fx['bn_absmax64'] = {k: float(v.abs().max()) for k, v in model3.state_dict().items() if 'running_' in k}
    print('exactly-zero statistics:', [k for k, v in fx['bn_buffers'].items() if fx['bn_absmax64'][k] < 1e-3 * float(v.abs().max())])
    print('exactly-zero gradients:', [k for k, n in fx['grad_norm'].items() if fx['grad_norm64'][k] < 1e-3 * n])
    torch.save(fx, OUT)
    print('out', tuple(out.shape), 'loss', fx['loss'], 'params with gradient', len(fx['grad_norm']), 'bf16 deviation', fx['bf16_dev'],
          'bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
