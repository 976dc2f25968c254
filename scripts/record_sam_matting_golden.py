"""Records tests/golden/sam_matting_tiny.pt by RUNNING THE REFERENCE implementation on the CPU in fp32.  The fixture holds recorded
tensors, names and settings only; every input is regenerated from a seed by the recipes of tests/sammat_common.py.

  loss_cases  {(kind, B, M, H, W): {loss key: value}} -- the reference's SAMMattingLoss (kind 'best': supervise_all_iou=True,
              'best_one_iou': False) and SAMMattingMultiLevelLoss ('multilevel') on group_inputs at the loss and Laplacian shapes,
              and 'best_index' per case: the arg-min the reference took
  lap_dev     {(B, M, H, W, masked): {'loss', 'grad'}}, at the Laplacian and the loss shapes -- how far the reference's own fp32 grouped Laplacian table and its gradient
              lie from the float64 judge (the largest relative deviation of a (b, m) entry; gradient relative to its largest element)
  model       per mask_out_idxs case ('all', 'subset'): config, image_size, keys (sorted state_dict names with shapes), init_sample
              (16 points of every initial floating tensor), out (strided samples of global / local / fused and iou_preds), out_stride,
              losses (the eight losses of SAMMattingLoss and of SAMMattingMultiLevelLoss on those outputs), grad_norm / grad_sample
              for the sum of the ARGMAX-FREE losses of the multi-level loss (both trimap losses, both local losses: a pixel whose two
              largest global probabilities nearly tie may take the other branch of collaborative_matting on other arithmetic),
              bn_buffers after the two-pass step (the first pass plus one refinement pass through the decoder), tie_share, bf16_dev,
              combine ([B, M]: the sum of the seven matting tables of the full-resolution outputs, what the arg-min is taken of),
              near_kink (per ReLU of the FUSION heads, named by its block: the flat NCHW indices of the inputs that lie within 1e-5 of
              zero in the first forward, which branch the reference took there, and the input's shape -- the gates another
              implementation may take the other way; the gradients above hold at THESE gates),
              gate_effect (gates [(block, index)], start, key (positions in grad_keys), value: what each recorded gate, taken the other way alone in the
              reference's own fp32 step, moves every parameter's gradient by, in the GPU test's measure),
              grad_dev64 (per parameter: the deviation of the reference's own fp32 gradient samples from a float64 run of the same
              step, relative to the tensor's largest gradient element)

    python scripts/record_sam_matting_golden.py --reference /path/to/reference/checkout

No test imports this script."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'sam_matting_tiny.pt')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import matting_common as M  # noqa: E402
import sammat_common as S  # noqa: E402
from oracle.make_golden_sam import SAM_TINY  # noqa: E402
from scripts.record_pfan_matting_golden import _Stub, sample_idx  # noqa: E402

ARGMAX_FREE = (0, 1, 2, 3)
NEAR_KINK = 1e-5
OUT_STRIDE = 7


def tiny_config(image_size):
    cfg = dict(SAM_TINY)
    cfg['image_size'] = image_size
    return cfg


def targets_of(batch):
    return batch['mask'], batch['trimap'], batch['fg_map'], batch['bg_map']


def prompts_of(batch, with_mask):
    return {'prompt_point': batch['prompt_point'], 'prompt_box': batch['prompt_box'],
            'prompt_mask': batch['prompt_mask'] if with_mask else None}


def loss_values(loss, d):
    out = loss(d['image'], ([d['global_preds']], [d['local_preds']], [d['fused_preds']], [d['iou_preds']]),
               (d['alpha'], d['trimap'], d['fg'], d['bg']))
    return {k: float(v) for k, v in out.items()}


def reference_combine(loss, d):
    """[B, M]: the reference's sum of its seven matting tables (all weights 1), the quantity its arg-min is taken of"""
    tabs = [loss.compute_global_trimap_ce_loss(d['global_preds'], d['trimap']),
            loss.compute_global_trimap_iou_loss(d['global_preds'], d['trimap']),
            loss.compute_local_alpha_loss(d['local_preds'], d['alpha'], d['trimap']),
            loss.compute_local_laplacian_loss(d['local_preds'], d['alpha'], d['trimap']),
            loss.compute_fusion_alpha_loss(d['fused_preds'], d['alpha']),
            loss.compute_fusion_laplacian_loss(d['fused_preds'], d['alpha']),
            loss.compute_composition_loss(d['image'], d['alpha'], d['fg'], d['bg'], d['fused_preds'])]
    return sum(tabs)


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
    from SimpleAICV.interactive_segmentation import losses_matting as ref_losses
    from SimpleAICV.interactive_segmentation.models.segment_anything_matting import sam_matting as ref_models
    assert os.path.abspath(ref_losses.__file__).startswith(os.path.abspath(args.reference))

    fx = {'loss_cases': {}, 'best_index': {}, 'lap_dev': {}, 'model': {}}
    kinds = {'best': ref_losses.SAMMattingLoss(), 'best_one_iou': ref_losses.SAMMattingLoss(supervise_all_iou=False),
             'multilevel': ref_losses.SAMMattingMultiLevelLoss()}
    for case in S.LOSS_CASES + S.LAP_CASES:
        d = S.group_inputs(*case)
        for kind, loss in kinds.items():
            fx['loss_cases'][(kind,) + case] = loss_values(loss, d)
        fx['best_index'][case] = torch.argmin(reference_combine(kinds['best'], d), dim=-1)
    for case in S.LAP_CASES + S.LOSS_CASES:
        d = S.group_inputs(*case)
        B, Mk, H, W = case
        inv = S.lap_inverse_counts(H, W)
        for masked in (False, True):
            name = 'local_preds' if masked else 'fused_preds'
            leaf = d[name].clone().requires_grad_(True)
            loss = kinds['best']
            table = (loss.compute_local_laplacian_loss(leaf, d['alpha'], d['trimap']) if masked
                     else loss.compute_fusion_laplacian_loss(leaf, d['alpha'])) * B
            table.sum().backward()
            gs = inv.expand(6, B * Mk)
            j = S.lap_group_judge(d[name], d['alpha'], d['trimap'] if masked else None, None, gs)
            want = (j['sums'] * inv).sum(0).view(B, Mk)
            live = want > 0
            fx['lap_dev'][case + (masked,)] = {
                'loss': float(((table.detach().double() - want).abs()[live] / want[live]).max()),
                'grad': float((leaf.grad.double() - j['dpred']).abs().max() / j['dpred'].abs().max())}
    print('reference fp32 grouped Laplacian against the float64 judge:', fx['lap_dev'])

    for image_size in (128, 256):
        try:
            torch.manual_seed(0)
            ref_models.SAMMATTING(**tiny_config(image_size))(S.model_batch(image_size)['image'],
                                                              prompts_of(S.model_batch(image_size), False))
            break
        except Exception as e:                                                  # the reference does not take this size
            print('image_size', image_size, 'refused by the reference:', repr(e)[:200])
    print('image_size', image_size)
    batch = S.model_batch(image_size)
    for case, idxs in S.MODEL_CASES.items():
        cfg = tiny_config(image_size)
        torch.manual_seed(0)
        model = ref_models.SAMMATTING(**cfg)
        model.train()
        init = {k: v.clone() for k, v in model.state_dict().items()}
        near_kink, hooks = {}, []

        def note(name):
            def hook(mod, inp):
                x = inp[0].detach().flatten()
                at = (x.abs() < NEAR_KINK).nonzero().flatten()
                near_kink[name] = {'index': at.int(), 'positive': x[at] > 0, 'shape': tuple(inp[0].shape)}
            return hook
        for name, mod in model.fusion_pred_list.named_modules():
            if isinstance(mod, torch.nn.ReLU):
                hooks.append(mod.register_forward_pre_hook(note(name[:-len('.layer.2')])))
        outs = model(batch['image'], prompts_of(batch, False), mask_out_idxs=idxs)
        for h in hooks:
            h.remove()
        det = tuple(o.detach() for o in outs)
        # the second pass of the two-pass step: the refinement pass reads the first pass's embeddings and a mask prompt
        emb = model.forward_image_encoder(batch['image'])
        model.forward_prompt_encoder_mask_decoder(emb, prompts_of(batch, True), mask_out_idxs=idxs)
        multi = ref_losses.SAMMattingMultiLevelLoss()
        inputs = ([det[0]], [det[1]], [det[2]], [det[3]])
        losses = {'best': {k: float(v) for k, v in ref_losses.SAMMattingLoss()(batch['image'], inputs, targets_of(batch)).items()},
                  'multilevel': {k: float(v) for k, v in multi(batch['image'], inputs, targets_of(batch)).items()}}
        live = multi(batch['image'], ([outs[0]], [outs[1]], [outs[2]], [outs[3]]), targets_of(batch))
        model.zero_grad()
        sum(live[S.LOSS_KEYS[i]] for i in ARGMAX_FREE).backward()
        top2 = torch.sort(det[0], dim=2, descending=True)[0]
        rec = {
            'config': cfg, 'image_size': image_size, 'mask_out_idxs': idxs,
            'keys': [(k, tuple(v.shape)) for k, v in sorted(init.items())],
            'init_sample': {k: v.flatten()[sample_idx(v.numel())].clone() for k, v in init.items() if v.dtype.is_floating_point},
            'out_stride': OUT_STRIDE,
            'out': tuple(o[..., ::OUT_STRIDE, ::OUT_STRIDE].clone() for o in det[:3]) + (det[3].clone(),),
            'out_absmax': tuple(float(o.abs().max()) for o in det),
            'losses': losses,
            'grad_norm': {k: float(p.grad.norm()) for k, p in model.named_parameters() if p.grad is not None},
            'grad_sample': {k: p.grad.flatten()[sample_idx(p.numel())].clone() for k, p in model.named_parameters()
                            if p.grad is not None},
            'bn_buffers': {k: v.clone() for k, v in model.state_dict().items() if 'running_' in k},
            'tie_share': float(((top2[:, :, 0] - top2[:, :, 1]) < 2e-3).float().mean()),
            'near_kink': near_kink, 'near_kink_below': NEAR_KINK,
            'combine': reference_combine(ref_losses.SAMMattingLoss(), dict(
                global_preds=det[0], local_preds=det[1], fused_preds=det[2], alpha=batch['mask'], trimap=batch['trimap'],
                image=batch['image'], fg=batch['fg_map'], bg=batch['bg_map'])).double(),
        }
        torch.manual_seed(0)
        model2 = ref_models.SAMMATTING(**cfg)
        model2.train()
        with torch.autocast('cpu', dtype=torch.bfloat16):
            outs2 = model2(batch['image'], prompts_of(batch, False), mask_out_idxs=idxs)
        rec['bf16_dev'] = max(float((a.float() - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(outs2[:2], det[:2]))
        # float64 arbiter of the same step (the reference's .float() calls would round it to fp32; the four losses are the composed
        # formulas of this package, which follow the dtype of the predictions): how far the reference's OWN fp32 gradients lie from
        # float64, per tensor, as the GPU test measures its deviation (samples against the tensor's largest gradient element)
        from simpleaicv_pytorch_training_examples_amd.SimpleAICV.interactive_segmentation import losses_matting as own
        torch.manual_seed(0)
        model3 = ref_models.SAMMATTING(**cfg).double()
        model3.prompt_encoder.pe_layer.float()          # (it casts its coordinates with .to(torch.float); its table is a constant)
        model3.train()
        float_orig = torch.Tensor.float
        torch.Tensor.float = lambda self: self if self.dtype == torch.float64 else float_orig(self)
        try:
            b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
            outs3 = model3(b64['image'], prompts_of(b64, False), mask_out_idxs=idxs)
            tabs = own.composed_tables(outs3[0], outs3[1], outs3[2], outs3[3], b64['image'], b64['mask'], b64['trimap'],
                                       b64['fg_map'], b64['bg_map'], 0.5)
            sum((t / tabs[0].shape[0]).mean(dim=-1).sum() for t in tabs[:4]).backward()
        finally:
            torch.Tensor.float = float_orig
        g32 = dict(model.named_parameters())
        rec['grad_dev64'] = {}
        for k, p in model3.named_parameters():
            if p.grad is None or k not in rec['grad_norm']:
                continue
            idx = sample_idx(p.numel())
            scale = float(p.grad.abs().max())
            rec['grad_dev64'][k] = (float((g32[k].grad.flatten()[idx].double() - p.grad.flatten()[idx]).abs().max()) / scale
                                    if scale > 0 else 0.)
        print(case, 'reference fp32 gradients against float64, worst five:',
              sorted(rec['grad_dev64'].items(), key=lambda kv: -kv[1])[:5])
        # what ONE recorded gate is worth: the same fp32 step with that single ReLU taking the other branch, against the step as
        # recorded, per parameter in the measure of the GPU test (norm relative to the norm, samples relative to the tensor's largest
        # element); entries below 1e-5 are dropped; stored as one table (gates, start of each gate's run, positions in grad_keys, values).  A gate changes the gradients of what lies before it and of nothing else.
        relus = {name[:-len('.layer.2')]: mod for name, mod in model.fusion_pred_list.named_modules() if isinstance(mod, torch.nn.ReLU)}
        for mod in relus.values():
            mod.inplace = False
        rec['gate_effect'], rec['grad_keys'] = {}, sorted(rec['grad_norm'])
        place = {k: i for i, k in enumerate(rec['grad_keys'])}
        for name, near in near_kink.items():
            for at in near['index'].tolist():
                def other_branch(mod, inp, out, at=at):
                    gate = (inp[0] > 0).contiguous()
                    gate.view(-1)[at] = ~gate.view(-1)[at]
                    return inp[0] * gate
                handle = relus[name].register_forward_hook(other_branch)
                model.zero_grad()
                o = model(batch['image'], prompts_of(batch, False), mask_out_idxs=idxs)
                lv = multi(batch['image'], ([o[0]], [o[1]], [o[2]], [o[3]]), targets_of(batch))
                sum(lv[S.LOSS_KEYS[i]] for i in ARGMAX_FREE).backward()
                handle.remove()
                effect = {}
                for k, p in model.named_parameters():
                    if k not in rec['grad_norm'] or p.grad is None or rec['grad_dev64'].get(k, 0.) > 1.:
                        continue                                    # (a gradient that is rounding noise has no effect to speak of)
                    base = rec['grad_sample'][k]
                    scale = max(float(p.grad.abs().max()), float(base.abs().max()))
                    if scale == 0. or rec['grad_norm'][k] == 0.:
                        continue
                    e = max(abs(float(p.grad.norm()) - rec['grad_norm'][k]) / rec['grad_norm'][k],
                            float((p.grad.flatten()[sample_idx(p.numel())] - base).abs().max()) / scale)
                    if e >= 1e-5:
                        effect[k] = e
                rec['gate_effect'][(name, at)] = ([place[k] for k in effect], list(effect.values()))
        worth = sorted(((max(v[1], default=0.), k) for k, v in rec['gate_effect'].items()), reverse=True)
        # (one flat table: a tensor per gate would cost more in pickle headers than in numbers)
        gates = list(rec['gate_effect'])
        rec['gate_effect'] = {
            'gates': gates, 'dropped_below': 1e-5,
            'start': torch.tensor([0] + [len(rec['gate_effect'][g][0]) for g in gates]).cumsum(0).int(),
            'key': torch.tensor([i for g in gates for i in rec['gate_effect'][g][0]], dtype=torch.int16),
            'value': (torch.tensor([v for g in gates for v in rec['gate_effect'][g][1]]) * 1.001).half()}     # (rounded up)
        print(case, 'gates recorded', len(worth), 'largest effect of one gate on a tensor', worth[:3], 'median', worth[len(worth) // 2][0])
        fx['model'][case] = rec
        print(case, 'out', [tuple(o.shape) for o in det], 'losses', losses, 'params with gradient', len(rec['grad_norm']),
              'bf16 deviation', rec['bf16_dev'], 'tie share', rec['tie_share'])
    torch.save(fx, OUT)
    print('bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
