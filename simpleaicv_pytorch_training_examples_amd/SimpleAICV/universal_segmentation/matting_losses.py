"""UniversalMattingLoss -- drop-in for the reference's SimpleAICV/universal_segmentation/matting_losses.py
(Mask2FormerHungarianMatcher :20, UniversalMattingLoss :249): same constructor, same seven keys.

Two routes, chosen by the environment variable SAICV_UNIMAT_LOSS ('fused', the default, or 'composed'), or by the `route`
attribute of an instance:

  fused     ops.matting_match_cost (csrc/unimat.hip: every pair sum of the batch from one pass over the three prediction tensors,
            read in place in whichever memory order they have) -> ONE copy of the packed [Q, sum T_i] cost to the host -> scipy's
            linear_sum_assignment per image -> ops.take_rows on the three prediction tensors (its backward writes each full-size
            gradient once, in the predictions' own memory order, zeros in the unmatched rows) -> ops.trimap_stats, ops.alpha_loss
            and ops.laplacian_l1 (csrc/matting.hip) on the M matched rows -> the reference's means; the local alpha loss divides by
            the batch-wide sum w + 1.  class_loss is a weighted cross entropy over [B * Q, C] in torch ops.
  composed  the reference's formulas as torch ops on the device, image after image: the benchmark's other side, and the route taken
            whenever a target's size differs from the predictions' (the reference pads such targets with zeros) or the maps are
            smaller than the five pyramid levels of ops.laplacian_l1 need.

An image without objects makes the reference raise (a matcher over an empty list); here it contributes no pair.  With no matched
pair in the whole batch the six map terms are NaN, so a training loop's skip-batch branch fires.  `last_indices` holds the
assignment of the latest call: per image (query indices, target indices)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

from ... import ops
from ..human_matting import losses as map_losses

__all__ = [
    'UniversalMattingLoss',
]

MAP_TERMS = ('global_trimap_ce_loss', 'global_trimap_iou_loss', 'local_alpha_loss', 'local_laplacian_loss', 'fusion_alpha_loss',
             'fusion_laplacian_loss')


def default_route():
    route = os.environ.get('SAICV_UNIMAT_LOSS', 'fused')
    if route not in ('fused', 'composed'):
        raise ValueError(f"SAICV_UNIMAT_LOSS must be 'fused' or 'composed', got {route!r}")
    return route


def trimap_class(trimap):
    """255 -> 2, else anything > 2 -> 1, else the integer part: the reference's three rewrites in their order"""
    k = trimap.clone()
    k[k == 255] = 2
    k[k > 2] = 1
    return k.long()


def composed_cost(pred_global, pred_local, pred_fused, pred_probs, trimap, alpha, labels, ce_cost, iou_cost, local_cost, fusion_cost,
                  class_cost):
    """The reference's cost matrix of one image: pred_global [Q, 3, H, W], pred_local / pred_fused [Q, H, W], pred_probs [Q, C],
    trimap / alpha [T, H, W] -> [Q, T]"""
    g = torch.clamp(pred_global.permute(0, 2, 3, 1), min=1e-4, max=1. - 1e-4)                   # [Q, H, W, 3]
    l = torch.clamp(pred_local, min=1e-4, max=1. - 1e-4)
    f = torch.clamp(pred_fused, min=1e-4, max=1. - 1e-4)
    classes = trimap_class(trimap)
    columns = []
    for t in range(trimap.shape[0]):
        onehot = F.one_hot(classes[t], num_classes=3).to(g.dtype)                               # [H, W, 3]
        ce = (-(onehot * torch.log(g) + (1. - onehot) * torch.log(1. - g))).mean(dim=(1, 2, 3))
        inter = (g * onehot).sum(dim=(1, 2, 3))
        union = g.sum(dim=(1, 2, 3)) + onehot.sum() - inter
        iou = 1. - (inter + 1e-4) / (union + 1e-4)
        w = (trimap[t] == 128).to(g.dtype)
        local = (torch.abs(l - alpha[t]) * w).sum(dim=(1, 2)) / (w.sum() + 1.)
        fusion = torch.abs(f - alpha[t]).mean(dim=(1, 2))
        columns.append(ce_cost * ce + iou_cost * iou + local_cost * local + fusion_cost * fusion)
    cost = torch.stack(columns, dim=1) if columns else g.new_zeros((g.shape[0], 0))
    cost = cost + class_cost * (-pred_probs[:, labels])
    return torch.nan_to_num(torch.clamp(cost, min=-1e10, max=1e10), 0)


class UniversalMattingLoss(nn.Module):

    def __init__(self, global_trimap_ce_cost=1.0, global_trimap_iou_cost=1.0, local_alpha_cost=1.0, fusion_alpha_cost=1.0,
                 class_cost=1.0, num_classes=2, global_trimap_ce_loss_weight=1.0, global_trimap_iou_loss_weight=1.0,
                 local_alpha_loss_weight=1.0, local_laplacian_loss_weight=1.0, fusion_alpha_loss_weight=1.0,
                 fusion_laplacian_loss_weight=1.0, class_loss_weight=1.0, no_object_class_weight=0.1):
        super(UniversalMattingLoss, self).__init__()
        self.num_classes = num_classes              # counts the background class, the last one
        self.costs = (global_trimap_ce_cost, global_trimap_iou_cost, local_alpha_cost, fusion_alpha_cost, class_cost)
        self.global_trimap_ce_loss_weight = global_trimap_ce_loss_weight
        self.global_trimap_iou_loss_weight = global_trimap_iou_loss_weight
        self.local_alpha_loss_weight = local_alpha_loss_weight
        self.local_laplacian_loss_weight = local_laplacian_loss_weight
        self.fusion_alpha_loss_weight = fusion_alpha_loss_weight
        self.fusion_laplacian_loss_weight = fusion_laplacian_loss_weight
        self.class_loss_weight = class_loss_weight
        self.register_buffer("ce_loss_weight", torch.ones(self.num_classes))
        self.ce_loss_weight[-1].fill_(no_object_class_weight)
        self.route = None                           # None: SAICV_UNIMAT_LOSS at call time
        self.last_indices = None
        # the six map terms are the human-matting losses on the matched rows (the reference repeats their code here)
        self.map_terms = (map_losses.GlobalTrimapCELoss(), map_losses.GloabelTrimapIouLoss(), map_losses.LocalAlphaLoss(),
                          map_losses.LocalLaplacianLoss(), map_losses.FusionAlphaLoss(), map_losses.FusionLaplacianLoss())

    # ------------------------------------------------------------------ matching
    @torch.no_grad()
    def match_fused(self, global_preds, local_preds, fused_preds, class_preds, trimaps, alphas, offsets, labels):
        cost = ops.matting_match_cost(global_preds, local_preds, fused_preds, class_preds, trimaps, alphas, offsets, labels,
                                      *self.costs).cpu()
        return [linear_sum_assignment(cost[:, offsets[i]:offsets[i + 1]]) for i in range(len(offsets) - 1)]

    @torch.no_grad()
    def match_composed(self, global_preds, local_preds, fused_preds, class_preds, trimap_gts, alpha_gts, class_gts):
        indices = []
        for i in range(global_preds.shape[0]):
            cost = composed_cost(global_preds[i], local_preds[i].squeeze(1), fused_preds[i].squeeze(1), class_preds[i].softmax(dim=-1),
                                 trimap_gts[i].to(global_preds), alpha_gts[i].to(global_preds), class_gts[i], *self.costs)
            indices.append(linear_sum_assignment(cost.cpu()))
        return indices

    # ------------------------------------------------------------------ terms
    def class_term(self, class_preds, labels, pair_b, pair_q, pair_t):
        b, q, c = class_preds.shape
        class_targets = torch.full((b, q), self.num_classes - 1, dtype=torch.int64, device=class_preds.device)
        class_targets[pair_b, pair_q] = labels[pair_t]
        return F.cross_entropy(class_preds.reshape(b * q, c), class_targets.reshape(-1), weight=self.ce_loss_weight.to(class_preds.dtype))

    def forward(self, global_preds, local_preds, fused_preds, class_preds, trimap_gts, alpha_gts, class_gts):
        device = fused_preds.device
        keep = torch.float32
        global_preds, local_preds, fused_preds, class_preds = (t.to(keep) for t in (global_preds, local_preds, fused_preds, class_preds))
        trimap_gts = [t.to(device=device, dtype=keep) for t in trimap_gts]
        alpha_gts = [t.to(device=device, dtype=keep) for t in alpha_gts]
        class_gts = [t.long().to(device) for t in class_gts]
        h, w = global_preds.shape[3], global_preds.shape[4]
        route = self.route or default_route()
        if (not global_preds.is_cuda or min(h, w) < ops.LAP_MIN_SIDE
                or any(tuple(t.shape[1:]) != (h, w) for t in trimap_gts + alpha_gts)):
            route = 'composed'
        offsets = [0]
        for t in trimap_gts:
            offsets.append(offsets[-1] + int(t.shape[0]))
        labels = torch.cat(class_gts) if class_gts else torch.zeros(0, dtype=torch.int64, device=device)

        if route == 'fused':
            empty = torch.zeros((0, h, w), device=device)
            trimaps = torch.cat(trimap_gts) if offsets[-1] else empty
            alphas = torch.cat(alpha_gts) if offsets[-1] else empty
            indices = self.match_fused(global_preds.detach(), local_preds.detach(), fused_preds.detach(), class_preds.detach(), trimaps,
                                       alphas, offsets, labels)
        else:
            indices = self.match_composed(global_preds.detach(), local_preds.detach(), fused_preds.detach(), class_preds.detach(),
                                          trimap_gts, alpha_gts, class_gts)
        self.last_indices = indices

        pb = torch.cat([torch.full((len(qi), ), i, dtype=torch.int64) for i, (qi, _) in enumerate(indices)]).to(device)
        pq = torch.cat([torch.as_tensor(qi, dtype=torch.int64) for qi, _ in indices]).to(device)
        pt = torch.cat([torch.as_tensor(ti, dtype=torch.int64) + offsets[i] for i, (_, ti) in enumerate(indices)]).to(device)
        m = int(pb.numel())

        if m == 0:
            terms = [torch.full((), float('nan'), device=device)] * 6
        else:
            if route == 'fused':
                mg, ml, mf = (ops.take_rows(t, pb, pq) for t in (global_preds, local_preds, fused_preds))
                mt, ma = trimaps[pt], alphas[pt]
            else:
                mg, ml, mf = global_preds[pb, pq], local_preds[pb, pq], fused_preds[pb, pq]
                hmax, wmax = max(t.shape[1] for t in trimap_gts), max(t.shape[2] for t in trimap_gts)
                padded = torch.zeros((2, offsets[-1], hmax, wmax), dtype=keep, device=device)
                for i, (tri, alp) in enumerate(zip(trimap_gts, alpha_gts)):
                    padded[0, offsets[i]:offsets[i + 1], :tri.shape[1], :tri.shape[2]] = tri
                    padded[1, offsets[i]:offsets[i + 1], :alp.shape[1], :alp.shape[2]] = alp
                mt, ma = padded[0, pt], padded[1, pt]
            for term in self.map_terms:
                term.route = route
            ce, iou, local_alpha, local_lap, fusion_alpha, fusion_lap = self.map_terms
            terms = [ce(mg, mt), iou(mg, mt), local_alpha(ml, ma, mt), local_lap(ml, ma, mt), fusion_alpha(mf, ma), fusion_lap(mf, ma)]
        class_loss = self.class_term(class_preds, labels, pb, pq, pt)

        weights = (self.global_trimap_ce_loss_weight, self.global_trimap_iou_loss_weight, self.local_alpha_loss_weight,
                   self.local_laplacian_loss_weight, self.fusion_alpha_loss_weight, self.fusion_laplacian_loss_weight)
        out = {name: wgt * value for name, wgt, value in zip(MAP_TERMS, weights, terms)}
        out['class_loss'] = self.class_loss_weight * class_loss
        return out
