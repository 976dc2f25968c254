"""Records tests/golden/pfan_sal_r18_tiny.pt by RUNNING THE REFERENCE implementation on the CPU in fp32.  The fixture holds recorded
tensors, names and settings only; every input is regenerated from a seed by the recipes of tests/salient_common.py.

  model   resnet18_pfan_segmentation (SimpleAICV/salient_object_detection/models/pfan_segmentation.py) built under
          torch.manual_seed(0), train mode, a seeded batch of 2 x 3 x 64 x 96 and a seeded soft mask:
          config, input_shape, keys (sorted state_dict names with shapes), init_sample (16 points of every initial floating tensor),
          out (the probabilities), losses (BCELoss, OHEMBCELoss, BCEIouloss, BCEDiceLoss of that output), grad_norm / grad_sample of
          every parameter for BCELoss + BCEIouloss, bn_buffers (running statistics after the step), bf16_dev (how far the reference's
          own bf16-autocast output moves from its fp32 output), grad_norm64 / bn_absmax64 (the same step in float64: which gradients
          and running means are exactly zero, see scripts/record_pfan_golden.py)
  losses  loss_cases: {(B, P): {loss name: value}} -- the reference BCELoss / BCEIouloss / BCEDiceLoss on pred [B, 1, P, 1]
  eval    the reference EvalMeter (tools/salient_object_detection_scripts.py:24-88) on two seeded batches with thresh [0.2, 0.5]

    python scripts/record_pfan_salient_golden.py --reference /path/to/reference/checkout

The reference packages import cv2 / torchvision / pycocotools / tqdm / thop / calflops at module scope for dataset and profiling
code; empty stand-ins are registered first.  No test imports this script."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'pfan_sal_r18_tiny.pt')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import salient_common as S  # noqa: E402

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
    from SimpleAICV.salient_object_detection.models import pfan_segmentation as ref_models
    from SimpleAICV.salient_object_detection import losses as ref_losses
    from tools.salient_object_detection_scripts import EvalMeter

    x, mask = S.model_inputs((BATCH, 3, H, W))

    def step(dtype):
        torch.manual_seed(0)
        model = ref_models.resnet18_pfan_segmentation(**CONFIG).to(dtype)
        model.train()
        init = {k: v.clone() for k, v in model.state_dict().items()}
        out = model(x.to(dtype))
        if dtype == torch.float64:
            out = out.double()                      # (the reference's pred.float() would round the float64 arbiter to fp32)
        return model, init, out

    model, init, out = step(torch.float32)
    assert out.dtype == torch.float32 and tuple(out.shape) == (BATCH, 1, H, W)
    losses = {name: float(ref_losses.__dict__[name]()(out.detach(), mask)) for name in ref_losses.__all__}
    (ref_losses.BCELoss()(out, mask) + ref_losses.BCEIouloss()(out, mask)).backward()
    fx = {
        'config': CONFIG, 'input_shape': (BATCH, 3, H, W),
        'keys': [(k, tuple(v.shape)) for k, v in sorted(init.items())],
        'init_sample': {k: v.flatten()[sample_idx(v.numel())].clone() for k, v in init.items() if v.dtype.is_floating_point},
        'out': out.detach().clone(), 'losses': losses,
        'grad_norm': {k: float(p.grad.norm()) for k, p in model.named_parameters() if p.grad is not None},
        'grad_sample': {k: p.grad.flatten()[sample_idx(p.numel())].clone() for k, p in model.named_parameters() if p.grad is not None},
        'bn_buffers': {k: v.clone() for k, v in model.state_dict().items() if 'running_' in k},
    }
    torch.manual_seed(0)
    model2 = ref_models.resnet18_pfan_segmentation(**CONFIG)
    model2.train()
    with torch.autocast('cpu', dtype=torch.bfloat16):
        out2 = model2(x)
    fx['bf16_dev'] = float((out2.float() - out.detach()).abs().max() / out.detach().abs().max().clamp_min(1e-30))

    # float64 arbiter: the reference forward ends in pred.float(), so the float64 step stops in front of it and applies the two
    # loss formulas in float64 by hand (clamp, log, sums -- losses.py:16-38 and :80-106)
    torch.manual_seed(0)
    model3 = ref_models.resnet18_pfan_segmentation(**CONFIG).double()
    model3.train()
    float_orig = torch.Tensor.float
    torch.Tensor.float = lambda self: self if self.dtype == torch.float64 else float_orig(self)
    try:
        out3 = model3(x.double())
        assert out3.dtype == torch.float64
        (ref_losses.BCELoss()(out3, mask.double()) + ref_losses.BCEIouloss()(out3, mask.double())).backward()
    finally:
        torch.Tensor.float = float_orig
    fx['grad_norm64'] = {k: float(p.grad.norm()) for k, p in model3.named_parameters() if p.grad is not None}
    fx['bn_absmax64'] = {k: float(v.abs().max()) for k, v in model3.state_dict().items() if 'running_' in k}
    print('exactly-zero statistics:', [k for k, v in fx['bn_buffers'].items() if fx['bn_absmax64'][k] < 1e-3 * float(v.abs().max())])
    print('exactly-zero gradients:', [k for k, n in fx['grad_norm'].items() if fx['grad_norm64'][k] < 1e-3 * n])

    fx['loss_cases'] = {}
    worst = 0.
    for B, P in S.LOSS_CASES:
        p, label = S.loss_inputs(B, P)
        vals = {name: float(ref_losses.__dict__[name]()(p.view(B, 1, P, 1), label.view(B, P, 1))) for name in S.LOSS_NAMES}
        fx['loss_cases'][(B, P)] = vals
        judge = S.stats_judge(p, label)['stats']
        for name in S.LOSS_NAMES:
            want = float(S.loss_from_stats(judge, P, name))
            worst = max(worst, abs(vals[name] - want) / max(1., abs(want)) / float(np.finfo(np.float32).eps))
    print(f'reference fp32 losses against the float64 judge: worst {worst:.2f} fp32 epsilons')

    class cfg:
        thresh, squared_beta = S.EVAL_THRESH, S.EVAL_SQUARED_BETA
    meter = EvalMeter(cfg)
    for preds, masks in S.eval_inputs():
        meter.add_batch_result(preds, masks)
    meter.compute_all_metrics()
    fx['eval'] = {k: (np.asarray(getattr(meter, k)).tolist()) for k in S.EVAL_KEYS}
    torch.save(fx, OUT)
    print('out', tuple(out.shape), 'losses', losses, 'params with gradient', len(fx['grad_norm']), 'bf16 deviation', fx['bf16_dev'],
          'eval', fx['eval'], 'bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
