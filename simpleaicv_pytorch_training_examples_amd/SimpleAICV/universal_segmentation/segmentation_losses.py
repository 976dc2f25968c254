"""UniversalSegmentationLoss -- drop-in for the reference's SimpleAICV/universal_segmentation/segmentation_losses.py
(Mask2FormerHungarianMatcher :16, UniversalSegmentationLoss :113): same constructor, same {'mask_loss', 'dice_loss', 'class_loss'}.

Two routes, chosen by the environment variable SAICV_UNIVSEG_LOSS ('fused', the default, or 'composed'), or by the `route`
attribute of an instance:

  fused     ops.mask_match_cost (csrc/univseg.hip: every pair sum of the batch from one pass over the logits, bf16 or fp32, read
            in place) -> ONE copy of the packed [Q, sum T_i] cost to the host -> scipy's linear_sum_assignment per image ->
            ops.matched_mask_stats (the four pixel sums of every matched pair through index tables; its backward writes the whole
            [B, Q, H, W] gradient, zeros in the unmatched rows) -> the two means.  class_loss is a weighted cross entropy over
            [B * Q, C] in torch ops.
  composed  the reference's formulas as torch ops on the device, image after image: the benchmark's other side, and the route
            taken whenever a target mask's size differs from the predictions' (the reference pads such targets with zeros).

With no matched pair in the batch both mask terms are NaN, as in the reference (a mean over nothing), so a training loop's
skip-batch branch fires.  `last_indices` holds the assignment of the latest call: per image (query indices, target indices)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

from ... import ops

__all__ = [
    'UniversalSegmentationLoss',
]


def default_route():
    route = os.environ.get('SAICV_UNIVSEG_LOSS', 'fused')
    if route not in ('fused', 'composed'):
        raise ValueError(f"SAICV_UNIVSEG_LOSS must be 'fused' or 'composed', got {route!r}")
    return route


def composed_cost(pred_mask, pred_probs, target_mask, labels, mask_cost, dice_cost, class_cost):
    """The reference's cost matrix of one image: pred_mask [Q, P] logits, pred_probs [Q, C], target_mask [T, P] -> [Q, T]"""
    hw = pred_mask.shape[1]
    pos = F.binary_cross_entropy_with_logits(pred_mask, torch.ones_like(pred_mask), reduction='none')
    neg = F.binary_cross_entropy_with_logits(pred_mask, torch.zeros_like(pred_mask), reduction='none')
    mask = torch.matmul(pos / hw, target_mask.T) + torch.matmul(neg / hw, (1 - target_mask).T)
    prob = torch.sigmoid(pred_mask)
    dice = 1 - (2 * torch.matmul(prob, target_mask.T) + 1) / (prob.sum(dim=-1)[:, None] + target_mask.sum(dim=-1)[None, :] + 1)
    cost = mask_cost * mask + dice_cost * dice + class_cost * (-pred_probs[:, labels])
    cost = torch.minimum(cost, torch.tensor(1e10))
    cost = torch.maximum(cost, torch.tensor(-1e10))
    return torch.nan_to_num(cost, 0)


class UniversalSegmentationLoss(nn.Module):

    def __init__(self, mask_cost=5.0, dice_cost=5.0, class_cost=2.0, num_classes=151, mask_loss_weight=5.0, dice_loss_weight=5.0,
                 class_loss_weight=2.0, no_object_class_weight=0.1):
        super(UniversalSegmentationLoss, self).__init__()
        self.num_classes = num_classes              # counts the background class, the last one
        self.mask_cost, self.dice_cost, self.class_cost = mask_cost, dice_cost, class_cost
        self.mask_loss_weight = mask_loss_weight
        self.dice_loss_weight = dice_loss_weight
        self.class_loss_weight = class_loss_weight
        self.register_buffer("ce_loss_weight", torch.ones(self.num_classes))
        self.ce_loss_weight[-1].fill_(no_object_class_weight)
        self.route = None                           # None: SAICV_UNIVSEG_LOSS at call time
        self.last_indices = None

    # ------------------------------------------------------------------ matching
    @torch.no_grad()
    def match_fused(self, mask_preds, class_preds, targets, offsets, labels):
        cost = ops.mask_match_cost(mask_preds, class_preds, targets, offsets, labels, self.mask_cost, self.dice_cost,
                                   self.class_cost).cpu()
        return [linear_sum_assignment(cost[:, offsets[i]:offsets[i + 1]]) for i in range(len(offsets) - 1)]

    @torch.no_grad()
    def match_composed(self, mask_preds, class_preds, mask_gts, class_gts):
        indices = []
        for i in range(mask_preds.shape[0]):
            cost = composed_cost(mask_preds[i].flatten(1), class_preds[i].softmax(dim=-1), mask_gts[i].to(mask_preds).flatten(1),
                                 class_gts[i], self.mask_cost, self.dice_cost, self.class_cost)
            indices.append(linear_sum_assignment(cost.cpu()))
        return indices

    # ------------------------------------------------------------------ terms
    def class_term(self, class_preds, labels, pair_b, pair_q, pair_t):
        b, q, c = class_preds.shape
        class_targets = torch.full((b, q), self.num_classes - 1, dtype=torch.int64, device=class_preds.device)
        class_targets[pair_b, pair_q] = labels[pair_t]
        return F.cross_entropy(class_preds.reshape(b * q, c), class_targets.reshape(-1), weight=self.ce_loss_weight)

    def forward(self, mask_preds, class_preds, mask_gts, class_gts):
        device = mask_preds.device
        class_preds = class_preds.float()
        mask_gts = [t.float().to(device) for t in mask_gts]
        class_gts = [t.long().to(device) for t in class_gts]
        route = self.route or default_route()
        if any(tuple(t.shape[1:]) != tuple(mask_preds.shape[2:]) for t in mask_gts):
            route = 'composed'
        counts = [int(t.shape[0]) for t in mask_gts]
        offsets = [0]
        for n in counts:
            offsets.append(offsets[-1] + n)
        labels = torch.cat(class_gts) if class_gts else torch.zeros(0, dtype=torch.int64, device=device)

        if route == 'fused':
            if mask_preds.dtype not in (torch.float32, torch.bfloat16):
                mask_preds = mask_preds.float()
            targets = torch.cat(mask_gts) if offsets[-1] else torch.zeros((0, ) + tuple(mask_preds.shape[2:]), device=device)
            indices = self.match_fused(mask_preds.detach(), class_preds.detach(), targets, offsets, labels)
        else:
            mask_preds = mask_preds.float()
            indices = self.match_composed(mask_preds.detach(), class_preds.detach(), mask_gts, class_gts)
        self.last_indices = indices

        pb = torch.cat([torch.full((len(qi), ), i, dtype=torch.int64) for i, (qi, _) in enumerate(indices)])
        pq = torch.cat([torch.as_tensor(qi, dtype=torch.int64) for qi, _ in indices])
        pt = torch.cat([torch.as_tensor(ti, dtype=torch.int64) + offsets[i] for i, (_, ti) in enumerate(indices)])
        m = int(pb.numel())
        hw = mask_preds.shape[2] * mask_preds.shape[3]

        if route == 'fused':
            if m:
                stats = ops.matched_mask_stats(mask_preds, targets, pb, pq, pt)
                mask_loss = stats[:, 0].sum() / (m * hw)
                dice_loss = (1 - (2 * stats[:, 1] + 1) / (stats[:, 2] + stats[:, 3] + 1)).mean()
            else:
                mask_loss = torch.full((), float('nan'), device=device)
                dice_loss = torch.full((), float('nan'), device=device)
            pbd, pqd, ptd = pb.to(device), pq.to(device), pt.to(device)
        else:
            pbd, pqd, ptd = pb.to(device), pq.to(device), pt.to(device)
            pred_masks = mask_preds[pbd, pqd].flatten(1)
            hmax = max([t.shape[1] for t in mask_gts] + [0])
            wmax = max([t.shape[2] for t in mask_gts] + [0])
            padded = torch.zeros((offsets[-1], hmax, wmax), dtype=torch.float32, device=device)
            for i, t in enumerate(mask_gts):
                padded[offsets[i]:offsets[i + 1], :t.shape[1], :t.shape[2]] = t
            target_masks = padded[ptd].flatten(1)
            mask_loss = F.binary_cross_entropy_with_logits(pred_masks, target_masks, reduction='none').mean()
            prob = torch.sigmoid(pred_masks)
            numerator = 2 * (prob * target_masks).sum(dim=-1)
            denominator = prob.sum(dim=-1) + target_masks.sum(dim=-1)
            dice_loss = (1 - (numerator + 1) / (denominator + 1)).mean()
        class_loss = self.class_term(class_preds, labels, pbd, pqd, ptd)

        return {
            'mask_loss': self.mask_loss_weight * mask_loss,
            'dice_loss': self.dice_loss_weight * dice_loss,
            'class_loss': self.class_loss_weight * class_loss,
        }
