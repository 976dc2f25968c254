"""Records tests/golden/univseg_tiny.pt by RUNNING THE REFERENCE implementation on the CPU.  The fixture holds recorded tensors, names
and settings only; every input is regenerated from a seed by the recipes of tests/univseg_common.py.

  loss_cases  {case: {'cost': [per image fp32 [Q, T_i]], 'cost_dev': [per image: the largest distance of that matrix from the same
              reference code run in float64], 'indices': [(query ids, target ids)], 'losses': {name: value}, 'losses64': the
              float64 run's, 'margin': [per image: how far the optimal assignment's total lies below the best other one, relative]}}
              for U.LOSS_CASES with the reference's Mask2FormerHungarianMatcher and UniversalSegmentationLoss at U.LOSS_WEIGHTS
  model       one training-mode step of dinov3_vit_small_patch16_universal_segmentation(**U.MODEL_CFG) at batch 2, constructed
              under torch.manual_seed(0) and run under torch.manual_seed(1) (the RoPE rescale draw): keys (state_dict names with
              shapes, in order), init_sample / init_absmax (16 points of every initial tensor), mask_preds, class_preds, losses,
              indices, grad_norm / grad_absmax / grad_sample per parameter for the sum of the three losses; and from the same step
              in float64: out_dev64, losses64, grad_dev64 (per parameter, samples against the tensor's largest gradient element)

    python scripts/record_universal_segmentation_golden.py --reference /path/to/reference/checkout

A loss case whose assignment is decided by less than 1e-3 of its total stops the recording: give it another seed in
U.LOSS_SEEDS (no case is dropped).  No test imports this script."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'univseg_tiny.pt')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import univseg_common as U  # noqa: E402
from scripts.record_pfan_matting_golden import _Stub  # noqa: E402

MARGIN = 1e-3


def reference_costs(matcher, mask_preds, class_preds, mask_gts, class_gts):
    """the cost matrices Mask2FormerHungarianMatcher.forward hands to scipy, by its own methods and its own clamping"""
    costs = []
    for i in range(mask_preds.shape[0]):
        probs = class_preds[i].softmax(dim=-1)
        pred, target = mask_preds[i].flatten(1), mask_gts[i].to(mask_preds[i]).flatten(1)
        cost = (matcher.mask_cost * matcher.compute_pair_wise_sigmoid_cross_entropy_loss(pred, target)
                + matcher.dice_cost * matcher.compute_pair_wise_dice_loss(pred, target)
                + matcher.class_cost * (-probs[:, class_gts[i]]))
        cost = torch.minimum(cost, torch.tensor(1e10))
        cost = torch.maximum(cost, torch.tensor(-1e10))
        costs.append(torch.nan_to_num(cost, 0))
    return costs


class keep_float64:
    """the reference casts with .float(): inside this block a float64 tensor stays what it is"""

    def __enter__(self):
        self.orig = torch.Tensor.float
        orig = self.orig
        torch.Tensor.float = lambda t: t if t.dtype == torch.float64 else orig(t)

    def __exit__(self, *a):
        torch.Tensor.float = self.orig


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
    for name in [n for n in sys.modules if n == 'SimpleAICV' or n.startswith('SimpleAICV.') or n == 'tools' or n.startswith('tools.')]:
        del sys.modules[name]
    from SimpleAICV.universal_segmentation import segmentation_losses as ref_losses
    from SimpleAICV.universal_segmentation.models import dinov3_universal_segmentation as ref_models
    assert os.path.abspath(ref_losses.__file__).startswith(os.path.abspath(args.reference))

    fx = {'loss_cases': {}, 'loss_weights': dict(U.LOSS_WEIGHTS)}
    for case in U.LOSS_CASES:
        C = case[5]
        x, cp, targets, labels = U.loss_inputs(case)
        crit = ref_losses.UniversalSegmentationLoss(num_classes=C, **U.LOSS_WEIGHTS)
        costs = reference_costs(crit.hungarian_matcher, x, cp, targets, labels)
        indices = crit.hungarian_matcher(x, cp, targets, labels)
        losses = {k: float(v) for k, v in crit(x, cp, targets, labels).items()}
        with keep_float64():
            crit64 = ref_losses.UniversalSegmentationLoss(num_classes=C, **U.LOSS_WEIGHTS).double()
            t64 = [t.double() for t in targets]
            costs64 = reference_costs(crit64.hungarian_matcher, x.double(), cp.double(), t64, labels)
            losses64 = {k: float(v) for k, v in crit64(x.double(), cp.double(), t64, labels).items()}
        margins = [float(U.assignment_margin(c)) if c.numel() else float('inf') for c in costs64]
        assert min(margins) >= MARGIN, f'{case}: an assignment is decided by {min(margins):.2e} only; change its seed in U.LOSS_SEEDS'
        fx['loss_cases'][U.case_id(case)] = {
            'cost': costs, 'cost_dev': [float((a.double() - b).abs().max()) if a.numel() else 0. for a, b in zip(costs, costs64)],
            'indices': [(q.clone(), t.clone()) for q, t in indices], 'losses': losses, 'losses64': losses64, 'margin': margins}
        print(case, losses, 'cost_dev', fx['loss_cases'][U.case_id(case)]['cost_dev'], 'margin', margins)

    images, masks, labels = U.model_batch()
    name = 'dinov3_vit_small_patch16_universal_segmentation'

    def step(dtype):
        torch.manual_seed(0)
        model = ref_models.__dict__[name](**U.MODEL_CFG)
        init = {k: v.clone() for k, v in model.state_dict().items()}
        model = model.to(dtype).train()
        crit = ref_losses.UniversalSegmentationLoss(num_classes=U.MODEL_CFG['num_classes'], **U.LOSS_WEIGHTS).to(dtype)
        torch.manual_seed(1)
        mask_preds, class_preds = model(images.to(dtype))
        out = crit(mask_preds, class_preds, [m.to(dtype) for m in masks], labels)
        sum(out.values()).backward()
        indices = crit.hungarian_matcher(mask_preds.detach(), class_preds.detach(), [m.to(dtype) for m in masks], labels)
        return model, init, mask_preds.detach(), class_preds.detach(), {k: float(v.detach()) for k, v in out.items()}, indices

    model, init, mp, cp, losses, indices = step(torch.float32)
    with keep_float64():
        model64, _, mp64, cp64, losses64, indices64 = step(torch.float64)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(indices, indices64))
    g32 = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    g64 = {k: p.grad for k, p in model64.named_parameters() if p.grad is not None}
    rec = {
        'name': name, 'config': dict(U.MODEL_CFG),
        'keys': [(k, tuple(v.shape)) for k, v in init.items()],
        'init_sample': {k: v.flatten()[U.sample_idx(v.numel())].clone() for k, v in init.items()},
        'init_absmax': {k: float(v.abs().max()) for k, v in init.items()},
        'mask_preds': mp.clone(), 'class_preds': cp.clone(), 'losses': losses, 'losses64': losses64,
        'indices': [(q.clone(), t.clone()) for q, t in indices],
        'grad_norm': {k: float(g.norm()) for k, g in g32.items()},
        'grad_absmax': {k: float(g.abs().max()) for k, g in g32.items()},
        'grad_sample': {k: g.flatten()[U.sample_idx(g.numel())].clone() for k, g in g32.items()},
        'out_dev64': {'mask_preds': float((mp.double() - mp64).abs().max() / mp64.abs().max()),
                      'class_preds': float((cp.double() - cp64).abs().max() / cp64.abs().max())},
        'grad_dev64': {},
    }
    for k, g in g64.items():
        idx = U.sample_idx(g.numel())
        scale = float(g.abs().max())
        rec['grad_dev64'][k] = float((g32[k].flatten()[idx].double() - g.flatten()[idx]).abs().max()) / scale if scale > 0 else 0.
    print('model step: losses', losses, 'float64', losses64, 'out_dev64', rec['out_dev64'])
    print('reference fp32 gradients against float64, worst five:', sorted(rec['grad_dev64'].items(), key=lambda kv: -kv[1])[:5])
    fx['model'] = rec
    torch.save(fx, OUT)
    print('bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
