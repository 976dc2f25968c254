"""Records tests/golden/unimat_tiny.pt by RUNNING THE REFERENCE implementation on the CPU.  The fixture holds recorded tensors, names
and settings only; every input is regenerated from a seed by the recipes of tests/unimat_common.py.

  loss_cases  {case: {'cost': [per image fp32 [Q, T_i]], 'cost_dev': [per image: the largest distance of that matrix from the same
              reference code run in float64, relative to the largest entry], 'indices': [(query ids, target ids)], 'losses': {name:
              value}, 'losses64': the float64 run's, 'grad_dev': {dglobal, dlocal, dfused, dclass: how far the fp32 gradient of the
              summed losses lies from the float64 run's, relative to its largest element}, 'margin': [per image: how far the optimal assignment's total lies below the best
              other one, relative]}} for U.LOSS_CASES (planted predictions) with the reference's Mask2FormerHungarianMatcher and
              UniversalMattingLoss at U.LOSS_WEIGHTS
  model       one training-mode step of dinov3_vit_small_patch16_universal_matting(**U.MODEL_CFG) at batch 2, built under
              manual_seed(0), fed U.model_batch() (manual_seed(10)) and run under manual_seed(1): keys (state_dict names with shapes, in
              order), init_sample / init_absmax (16 points of every initial tensor), the four outputs, losses, indices, grad_norm /
              grad_absmax / grad_sample per parameter for the sum of the seven losses; from the same step in float64: out_dev64,
              losses64, grad_dev64, and `undecided` (the pixels whose two largest float64 global probabilities differ by less than
              U.UNDECIDED; they are left out of every fused_preds comparison), `fused_flipped` (decided pixels whose fp32 fused value
              is on the other side)

    python scripts/record_universal_matting_golden.py --reference /path/to/reference/checkout

A loss case whose assignment is decided by less than 1e-3 of its total stops the recording (give it another seed in U.LOSS_SEEDS; no
case is dropped), and so does a model step with more than 0.1 % undecided pixels.  In the float64 runs the reference's fp32 Gaussian
filter and its fp32 padded targets are cast to float64 at the convolution (which refuses mixed types).  No test imports this script."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'unimat_tiny.pt')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import unimat_common as U  # noqa: E402
from scripts.record_pfan_matting_golden import _Stub  # noqa: E402
from scripts.record_universal_segmentation_golden import keep_float64  # noqa: E402

MARGIN = 1e-3


def reference_costs(matcher, gp, lp, fp, class_preds, trimaps, alphas, labels):
    """the cost matrices Mask2FormerHungarianMatcher.forward hands to scipy, by its own methods and its own clamping"""
    costs = []
    for i in range(gp.shape[0]):
        probs = class_preds[i].softmax(dim=-1)
        tri, alp = trimaps[i].to(gp), alphas[i].to(gp)
        cost = (matcher.global_trimap_ce_cost * matcher.compute_pair_wise_trimap_ce_cost(gp[i], tri)
                + matcher.global_trimap_iou_cost * matcher.compute_pair_wise_trimap_iou_cost(gp[i], tri)
                + matcher.local_alpha_cost * matcher.compute_pair_wise_local_alpha_cost(lp[i].squeeze(1), alp, tri)
                + matcher.fusion_alpha_cost * matcher.compute_pair_wise_fusion_alpha_cost(fp[i].squeeze(1), alp)
                + matcher.class_cost * (-probs[:, labels[i]]))
        costs.append(torch.nan_to_num(torch.clamp(cost, min=-1e10, max=1e10), 0))
    return costs


def float64_filter(crit):
    conv = crit.conv_gauss
    crit.conv_gauss = lambda img, kernel: conv(img.double(), kernel.double())     # the padded targets are fp32 tensors, exactly
    return crit


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
    from SimpleAICV.universal_segmentation import matting_losses as ref_losses
    from SimpleAICV.universal_segmentation.models import dinov3_universal_matting as ref_models
    assert os.path.abspath(ref_losses.__file__).startswith(os.path.abspath(args.reference))

    fx = {'loss_cases': {}, 'loss_weights': dict(U.LOSS_WEIGHTS), 'loss_classes': U.LOSS_CLASSES}
    for case in U.LOSS_CASES:
        gp, lp, fp, cp, trimaps, alphas, labels = U.loss_inputs(case)
        crit = ref_losses.UniversalMattingLoss(num_classes=U.LOSS_CLASSES, **U.LOSS_WEIGHTS)
        costs = reference_costs(crit.hungarian_matcher, gp, lp, fp, cp, trimaps, alphas, labels)
        indices = crit.hungarian_matcher(gp, lp, fp, cp, trimaps, alphas, labels)
        leaves = [t.clone().requires_grad_(True) for t in (gp, lp, fp, cp)]
        out = crit(*leaves, trimaps, alphas, labels)
        sum(out.values()).backward()
        losses = {k: float(v.detach()) for k, v in out.items()}
        with keep_float64():
            crit64 = float64_filter(ref_losses.UniversalMattingLoss(num_classes=U.LOSS_CLASSES, **U.LOSS_WEIGHTS).double())
            t64, a64 = [t.double() for t in trimaps], [a.double() for a in alphas]
            costs64 = reference_costs(crit64.hungarian_matcher, gp.double(), lp.double(), fp.double(), cp.double(), t64, a64, labels)
            leaves64 = [t.double().requires_grad_(True) for t in (gp, lp, fp, cp)]
            out64 = crit64(*leaves64, t64, a64, labels)
            sum(out64.values()).backward()
            losses64 = {k: float(v.detach()) for k, v in out64.items()}
        grad_dev = [float((a.grad.double() - b.grad).abs().max() / b.grad.abs().max()) for a, b in zip(leaves, leaves64)]
        margins = [float(U.assignment_margin(c)) if c.numel() else float('inf') for c in costs64]
        assert min(margins) >= MARGIN, f'{case}: an assignment is decided by {min(margins):.2e} only; change its seed in U.LOSS_SEEDS'
        fx['loss_cases'][U.case_id(case)] = {
            'cost': costs,
            'cost_dev': [float((a.double() - b).abs().max() / b.abs().max()) if a.numel() else 0. for a, b in zip(costs, costs64)],
            'indices': [(q.clone(), t.clone()) for q, t in indices], 'losses': losses, 'losses64': losses64, 'margin': margins,
            'grad_dev': dict(zip(('dglobal', 'dlocal', 'dfused', 'dclass'), grad_dev))}
        print(case, losses, 'cost_dev', fx['loss_cases'][U.case_id(case)]['cost_dev'], 'margin', margins, 'grad_dev', grad_dev)

    images, trimaps, alphas, labels = U.model_batch()
    name = 'dinov3_vit_small_patch16_universal_matting'

    def step(dtype):
        torch.manual_seed(U.MODEL_SEEDS['build'])
        model = ref_models.__dict__[name](**U.MODEL_CFG)
        init = {k: v.clone() for k, v in model.state_dict().items()}
        model = model.to(dtype).train()
        crit = ref_losses.UniversalMattingLoss(num_classes=U.MODEL_CFG['num_classes'], **U.LOSS_WEIGHTS).to(dtype)
        if dtype == torch.float64:
            float64_filter(crit)
        torch.manual_seed(U.MODEL_SEEDS['run'])
        outs = model(images.to(dtype))
        tri, alp = [t.to(dtype) for t in trimaps], [a.to(dtype) for a in alphas]
        out = crit(*outs, tri, alp, labels)
        sum(out.values()).backward()
        indices = crit.hungarian_matcher(*[o.detach() for o in outs], tri, alp, labels)
        return model, init, [o.detach() for o in outs], {k: float(v.detach()) for k, v in out.items()}, indices

    model, init, outs, losses, indices = step(torch.float32)
    with keep_float64():
        model64, _, outs64, losses64, indices64 = step(torch.float64)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(indices, indices64))
    top = torch.topk(outs64[0], 2, dim=2)[0]
    undecided = ((top[:, :, 0:1] - top[:, :, 1:2]) < U.UNDECIDED)
    assert float(undecided.float().mean()) <= U.UNDECIDED_CAP, 'too many undecided pixels: take another seed'
    flipped = int(((outs[2].double() - outs64[2]).abs() > 1e-3)[~undecided].sum())
    g32 = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    g64 = {k: p.grad for k, p in model64.named_parameters() if p.grad is not None}
    names = ('global_preds', 'local_preds', 'fused_preds', 'class_preds')
    rec = {
        'name': name, 'config': dict(U.MODEL_CFG),
        'keys': [(k, tuple(v.shape)) for k, v in init.items()],
        'init_sample': {k: v.flatten()[U.sample_idx(v.numel())].clone() for k, v in init.items()},
        'init_absmax': {k: float(v.abs().max()) for k, v in init.items()},
        'losses': losses, 'losses64': losses64, 'indices': [(q.clone(), t.clone()) for q, t in indices],
        'undecided': undecided.nonzero().clone(), 'fused_flipped': flipped,
        'grad_norm': {k: float(g.norm()) for k, g in g32.items()},
        'grad_absmax': {k: float(g.abs().max()) for k, g in g32.items()},
        'grad_sample': {k: g.flatten()[U.sample_idx(g.numel())].clone() for k, g in g32.items()},
        'out_dev64': {}, 'grad_dev64': {},
    }
    for n, o, o64 in zip(names, outs, outs64):
        rec[n] = o.clone()
        keep = ~undecided.expand_as(o) if n == 'fused_preds' else torch.ones_like(o, dtype=torch.bool)
        rec['out_dev64'][n] = float(((o.double() - o64).abs() * keep).max() / o64.abs().max())
    for k, g in g64.items():
        idx = U.sample_idx(g.numel())
        scale = float(g.abs().max())
        rec['grad_dev64'][k] = float((g32[k].flatten()[idx].double() - g.flatten()[idx]).abs().max()) / scale if scale > 0 else 0.
    print('model step: losses', losses, 'float64', losses64, 'out_dev64', rec['out_dev64'], 'undecided', int(undecided.sum()),
          'flipped', flipped)
    print('reference fp32 gradients against float64, worst five:', sorted(rec['grad_dev64'].items(), key=lambda kv: -kv[1])[:5])
    fx['model'] = rec
    torch.save(fx, OUT)
    print('bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
