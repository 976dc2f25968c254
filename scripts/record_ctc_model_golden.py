"""Records tests/golden/ctc_model_r18_tiny.pt by RUNNING THE REFERENCE implementation on the CPU in fp32: CTCModel(backbone_type=
'resnet18backbone', planes=32, num_classes=40) (SimpleAICV/text_recognition/models/ctc_model.py) built under torch.manual_seed(0),
in train mode, on a seeded batch of 2 x 3 x 32 x 64, the reference CTCLoss (blank 38) on seeded targets, one backward.  Fields:
config, input_shape, keys (state_dict names and shapes), init_sample, out (the full logits), loss, grad_norm / grad_sample per
parameter, bn_buffers, targets / target_lengths.  The fixture holds recorded tensors, names and settings only.

    python scripts/record_ctc_model_golden.py --reference /path/to/reference/checkout

The reference packages import cv2 / torchvision / pycocotools / tqdm / thop / calflops at module scope for dataset and profiling
code; empty stand-ins are registered first.  No test imports this script; tests/test_gpu_text_recognition.py rebuilds the same
model under the same seed and compares."""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'ctc_model_r18_tiny.pt')

CONFIG = dict(backbone_type='resnet18backbone', backbone_pretrained_path='', planes=32, num_classes=40, use_gradient_checkpoint=False)
BATCH, H, W = 2, 32, 64
BLANK = 38


def sample_idx(numel, k=16):
    return torch.linspace(0, numel - 1, min(k, numel)).long()


def inputs():
    x = torch.randn(BATCH, H, W, 3, generator=torch.Generator().manual_seed(1)).permute(0, 3, 1, 2)      # NHWC memory
    targets = torch.full((BATCH, 6), BLANK, dtype=torch.long)
    targets[0, :3] = torch.tensor([5, 5, 39])            # a repeat and the garbage class
    targets[1, :2] = torch.tensor([0, 17])
    return x, targets, torch.IntTensor([3, 2])


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
    from SimpleAICV.text_recognition.losses import CTCLoss
    from SimpleAICV.text_recognition.models.ctc_model import CTCModel

    torch.manual_seed(0)
    model = CTCModel(**CONFIG)
    model.train()
    x, targets, target_lengths = inputs()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    out = model(x)
    input_lengths = torch.IntTensor([out.shape[1]] * BATCH)
    loss = CTCLoss(blank_index=BLANK)(out.permute(1, 0, 2), targets, input_lengths, target_lengths)
    loss.backward()
    fx = {
        'config': CONFIG, 'input_shape': (BATCH, 3, H, W), 'blank': BLANK, 'targets': targets, 'target_lengths': target_lengths,
        'keys': [(k, tuple(v.shape)) for k, v in sorted(init.items())],
        'init_sample': {k: v.flatten()[sample_idx(v.numel())].clone() for k, v in init.items() if v.dtype.is_floating_point},
        'out': out.detach().clone(), 'loss': float(loss.detach()),
        'grad_norm': {k: float(p.grad.norm()) for k, p in model.named_parameters() if p.grad is not None},
        'grad_sample': {k: p.grad.flatten()[sample_idx(p.numel())].clone() for k, p in model.named_parameters() if p.grad is not None},
        'bn_buffers': {k: v.clone() for k, v in model.state_dict().items() if 'running_' in k},
    }
    torch.save(fx, OUT)
    print('out', tuple(out.shape), 'loss', fx['loss'], 'params with gradient', len(fx['grad_norm']), 'bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
