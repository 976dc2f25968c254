"""Records tests/golden/pfan_parse_r18_tiny.pt by RUNNING THE REFERENCE implementation on the CPU in fp32.  Two parts:

(a) `step`: resnet18_pfan_human_parsing(num_classes=20) (SimpleAICV/human_parsing/models/pfan_human_parsing.py) built under
torch.manual_seed(0), in train mode, on a seeded batch of 2 x 3 x 64 x 64, the reference CELoss + IoULoss('softmax')
(human_parsing/losses.py:13-43, :79-113) on a seeded integer mask, and one backward of their sum.  The fields of
pfan_r18_tiny.pt (scripts/record_pfan_golden.py): config, input_shape, keys, init_sample, loss (here a dict per loss name),
out (the full prediction: the file stays below 1 MiB with it), grad_norm / grad_sample, bn_buffers, bf16_dev, grad_norm64,
bn_absmax64.

(b) `loss_values`: the reference CELoss, MultiClassBCELoss, IoULoss and DiceLoss (the last two with both logit types) on a seeded
fp32 logits tensor of 1 x 20 x 8 x 12 (`loss_logits`: a third of the pixels scaled by 1, 6 and 14, so that every clamp is
exercised) with seeded labels (`loss_labels`).  tests/test_parsing_host.py pins the float64 judge to these values.

The fixture holds recorded tensors, names and settings only.

    python scripts/record_pfan_parsing_golden.py --reference /path/to/reference/checkout

The reference packages import cv2 / torchvision / pycocotools / tqdm / thop / calflops at module scope for dataset and
profiling code; empty stand-ins are registered first.  No test imports this script; the product-side tests rebuild the same model
under the same seed and compare."""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'pfan_parse_r18_tiny.pt')

CONFIG = dict(num_classes=20)
BATCH, H, W = 2, 64, 64
LOSS_SHAPE = (1, 20, 8, 12)


def sample_idx(numel, k=16):
    return torch.linspace(0, numel - 1, min(k, numel)).long()


def inputs():
    x = torch.randn(BATCH, H, W, 3, generator=torch.Generator().manual_seed(1)).permute(0, 3, 1, 2)      # NHWC memory
    mask = torch.randint(0, CONFIG['num_classes'], (BATCH, H, W), generator=torch.Generator().manual_seed(2)).float()
    return x, mask


def loss_inputs():
    b, c, h, w = LOSS_SHAPE
    g = torch.Generator().manual_seed(3)
    scale = torch.tensor([1., 6., 14.])[torch.arange(b * h * w) % 3].view(b, 1, h, w)
    logits = torch.randn(b, c, h, w, generator=g) * scale
    labels = torch.randint(0, c, (b, h, w), generator=g).float()
    return logits, labels


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
    from SimpleAICV.human_parsing.models import pfan_human_parsing as ref_models
    from SimpleAICV.human_parsing.losses import CELoss, DiceLoss, IoULoss, MultiClassBCELoss

    def criterion(out, mask):
        return {'CELoss': CELoss()(out, mask), 'IoULoss': IoULoss(logit_type='softmax')(out, mask)}

    torch.manual_seed(0)
    model = ref_models.resnet18_pfan_human_parsing(**CONFIG)
    model.train()
    x, mask = inputs()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    out = model(x)
    loss = criterion(out, mask)
    sum(loss.values()).backward()
    fx = {
        'config': CONFIG, 'input_shape': (BATCH, 3, H, W),
        'keys': [(k, tuple(v.shape)) for k, v in sorted(init.items())],
        'init_sample': {k: v.flatten()[sample_idx(v.numel())].clone() for k, v in init.items() if v.dtype.is_floating_point},
        'out': out.detach().clone(),
        'loss': {k: float(v.detach()) for k, v in loss.items()},
        'grad_norm': {k: float(p.grad.norm()) for k, p in model.named_parameters() if p.grad is not None},
        'grad_sample': {k: p.grad.flatten()[sample_idx(p.numel())].clone() for k, p in model.named_parameters() if p.grad is not None},
        'bn_buffers': {k: v.clone() for k, v in model.state_dict().items() if 'running_' in k},
    }
    torch.manual_seed(0)
    model2 = ref_models.resnet18_pfan_human_parsing(**CONFIG)
    model2.train()
    with torch.autocast('cpu', dtype=torch.bfloat16):
        out2 = model2(x)
    fx['bf16_dev'] = float((out2.float() - out.detach()).abs().max() / out.detach().abs().max().clamp_min(1e-30))
    torch.manual_seed(0)
    model3 = ref_models.resnet18_pfan_human_parsing(**CONFIG).double()
    model3.train()
    sum(criterion(model3(x.double()), mask).values()).backward()
    fx['grad_norm64'] = {k: float(p.grad.norm()) for k, p in model3.named_parameters() if p.grad is not None}
    fx['bn_absmax64'] = {k: float(v.abs().max()) for k, v in model3.state_dict().items() if 'running_' in k}
    print('exactly-zero statistics:', [k for k, v in fx['bn_buffers'].items() if fx['bn_absmax64'][k] < 1e-3 * float(v.abs().max())])
    print('exactly-zero gradients:', [k for k, n in fx['grad_norm'].items() if fx['grad_norm64'][k] < 1e-3 * n])

    logits, labels = loss_inputs()
    fx['loss_logits'], fx['loss_labels'] = logits.clone(), labels.clone()
    fx['loss_values'] = {
        'softmax': [float(CELoss()(logits, labels)), float(IoULoss(logit_type='softmax')(logits, labels)),
                    float(DiceLoss(logit_type='softmax')(logits, labels))],
        'sigmoid': [float(MultiClassBCELoss()(logits, labels)), float(IoULoss(logit_type='sigmoid')(logits, labels)),
                    float(DiceLoss(logit_type='sigmoid')(logits, labels))],
    }
    torch.save(fx, OUT)
    print('out', tuple(out.shape), 'loss', fx['loss'], 'loss values', fx['loss_values'], 'params with gradient', len(fx['grad_norm']),
          'bf16 deviation', fx['bf16_dev'], 'bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
