"""Losses of the reference's SAM matting family (SimpleAICV/interactive_segmentation/losses_matting.py): same names, constructor
arguments, forward(images, inputs, targets) and the eight loss_dict keys.

inputs = (all_iter_global_preds, all_iter_local_preds, all_iter_fused_preds, all_iter_iou_preds): per decoder pass
[B, M, 3, H, W], [B, M, 1, H, W], [B, M, 1, H, W] probabilities and [B, M]; targets = (masks [B, 1, H, W] soft alpha, trimaps
[B, H, W] in {0, 128, 255}, fg_maps, bg_maps [B, 3, H, W]).

Every loss is a [B, M] table first (each entry divided by its own pixel count -- the local alpha loss by sum w + 1 of its own row --
and by B), then
  SAMMattingLoss            keeps, per sample, the mask with the smallest weighted sum of the seven matting losses when M > 1 (all
                            rows when M == 1); its IoU-prediction loss is the mean over M or the kept entry, by supervise_all_iou;
  SAMMattingMultiLevelLoss  takes the mean over M of everything.

route = 'fused' (the default: measured faster than 'composed' at both probed batch sizes, profiles/sam_matting_step.json): the tables
come from ops.group_matting_stats and ops.group_laplacian_sums (csrc/matting.hip): the targets are never
repeated M times, each target value is loaded once per pixel for all M masks, and the backward reads only the rows whose
coefficients are non-zero (one in M for SAMMattingLoss).  route = 'composed': the reference formulas as torch ops on the tensors'
device; CPU tensors always take it (host tests).  The [B, M]-sized arithmetic is torch on the device on both routes; nothing is read
back to the host.  `last_best_index` holds the kept mask per sample of the last decoder pass (SAMMattingLoss, M > 1; detached)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops

__all__ = [
    'SAMMattingLoss',
    'SAMMattingMultiLevelLoss',
]

LOSS_KEYS = ('global_pred_trimap_ce_loss', 'global_pred_trimap_iou_loss', 'local_pred_alpha_loss', 'local_pred_laplacian_loss',
             'fusion_pred_alpha_loss', 'fusion_pred_laplacian_loss', 'composition_loss', 'iou_predict_loss')
LO, HI = 1e-4, 1. - 1e-4


def _pyramid(x, kernel, levels=5):
    out = []
    for _ in range(levels):
        f = F.conv2d(F.pad(x, (2, 2, 2, 2), mode='replicate'), kernel, groups=kernel.shape[0])
        out.append(x - f)
        x = F.avg_pool2d(f, 2)
    return out + [x]


def _laplacian_table(pred, target):
    """pred, target [B, M, H, W] -> [B, M]: the sum over the six pyramid entries of their mean absolute difference"""
    m = pred.shape[1]
    k = torch.tensor(ops.laplacian_gauss_table(), dtype=pred.dtype, device=pred.device).view(1, 1, 5, 5).repeat(m, 1, 1, 1)
    total = 0.
    for a, b in zip(_pyramid(target, k), _pyramid(pred, k)):
        total = total + (a - b).abs().flatten(2).mean(dim=-1)
    return total


def composed_tables(global_preds, local_preds, fused_preds, iou_preds, images, masks, trimaps, fg_maps, bg_maps, mask_threshold):
    """the eight [B, M] tables by the reference's formulas (losses_matting.py:237-578) as torch ops, before the division by B"""
    gp = torch.clamp(global_preds.float(), min=LO, max=HI)                      # [B, M, 3, H, W]
    lp = torch.clamp(local_preds.float(), min=LO, max=HI).squeeze(2)            # [B, M, H, W]
    fp = torch.clamp(fused_preds.float(), min=LO, max=HI).squeeze(2)
    m = gp.shape[1]
    cls = trimaps.clone()
    cls[cls == 255] = 2
    cls[cls > 2] = 1
    onehot = F.one_hot(cls.long(), num_classes=3).permute(0, 3, 1, 2).float().unsqueeze(1)          # [B, 1, 3, H, W]
    bce = -(onehot * torch.log(gp) + (1. - onehot) * torch.log(1. - gp))
    ce = bce.flatten(2).mean(dim=-1)
    inter = (gp * onehot).sum(dim=2)
    iou = (1. - (inter + 1e-4) / (gp.sum(dim=2) + onehot.sum(dim=2) - inter + 1e-4)).flatten(2).mean(dim=-1)
    w = (trimaps == 128).float().unsqueeze(1)                                   # [B, 1, H, W]
    alpha = masks.float()                                                       # [B, 1, H, W]
    la = torch.sqrt(((lp - alpha) * w) ** 2 + 1e-12).sum(dim=[2, 3]) / (w.sum(dim=[2, 3]) + 1.)
    ll = _laplacian_table(lp * w, (alpha * w).expand(-1, m, -1, -1))
    fa = torch.sqrt((fp - alpha) ** 2 + 1e-12).flatten(2).mean(dim=-1)
    fl = _laplacian_table(fp, alpha.expand(-1, m, -1, -1))
    f3 = fp.unsqueeze(2)
    comp = f3 * fg_maps.float().unsqueeze(1) + (1. - f3) * bg_maps.float().unsqueeze(1)
    cl = torch.sqrt((comp - images.float().unsqueeze(1)) ** 2 + 1e-12).flatten(2).mean(dim=-1)
    pb, ab = fp > mask_threshold, alpha > mask_threshold
    gt = (pb & ab).flatten(2).sum(dim=-1).float() / torch.clamp((pb | ab).flatten(2).sum(dim=-1).float(), min=1e-6)
    ip = F.mse_loss(iou_preds.float(), torch.clamp(gt, min=0., max=1.), reduction='none')
    return [ce, iou, la, ll, fa, fl, cl, ip]


_lap_inv = {}


def _lap_inverse_counts(device, h, w):
    key = (device, h, w)
    if key not in _lap_inv:
        _lap_inv[key] = torch.tensor([1. / ((h >> l) * (w >> l)) for l in range(ops.LAP_LEVELS + 1)], dtype=torch.float32,
                                     device=device).view(-1, 1)
    return _lap_inv[key]


def fused_tables(global_preds, local_preds, fused_preds, iou_preds, images, masks, trimaps, fg_maps, bg_maps, mask_threshold):
    """the same eight tables from the grouped kernels"""
    b, m, _, h, w = global_preds.shape
    p = float(h * w)
    st = ops.group_matting_stats(global_preds, local_preds, fused_preds, masks, trimaps, images, fg_maps, bg_maps, mask_threshold)
    inv = _lap_inverse_counts(st.device, h, w)
    ll = (ops.group_laplacian_sums(local_preds, masks, trimaps) * inv).sum(dim=0).view(b, m)
    fl = (ops.group_laplacian_sums(fused_preds, masks) * inv).sum(dim=0).view(b, m)
    gt = st[..., 6] / torch.clamp(st[..., 7], min=1e-6)
    ip = F.mse_loss(iou_preds.float(), torch.clamp(gt, min=0., max=1.).detach(), reduction='none')
    return [st[..., 0] / (3. * p), st[..., 1] / p, st[..., 2] / (st[..., 3].detach() + 1.), ll, st[..., 4] / p, fl,
            st[..., 5] / (3. * p), ip]


class SAMMattingLoss(nn.Module):
    route = 'fused'
    reduce_all_masks = False

    def __init__(self,
                 global_pred_trimap_ce_loss_weight=1,
                 global_pred_trimap_iou_loss_weight=1,
                 local_pred_alpha_loss_weight=1,
                 local_pred_laplacian_loss_weight=1,
                 fusion_pred_alpha_loss_weight=1,
                 fusion_pred_laplacian_loss_weight=1,
                 composition_loss_weight=1,
                 iou_predict_loss_weight=1,
                 supervise_all_iou=True,
                 mask_threshold=0.5,
                 route=None):
        super(SAMMattingLoss, self).__init__()
        self.global_pred_trimap_ce_loss_weight = global_pred_trimap_ce_loss_weight
        self.global_pred_trimap_iou_loss_weight = global_pred_trimap_iou_loss_weight
        self.local_pred_alpha_loss_weight = local_pred_alpha_loss_weight
        self.local_pred_laplacian_loss_weight = local_pred_laplacian_loss_weight
        self.fusion_pred_alpha_loss_weight = fusion_pred_alpha_loss_weight
        self.fusion_pred_laplacian_loss_weight = fusion_pred_laplacian_loss_weight
        self.composition_loss_weight = composition_loss_weight
        self.iou_predict_loss_weight = iou_predict_loss_weight
        self.supervise_all_iou = supervise_all_iou
        self.mask_threshold = mask_threshold
        if route is not None:
            if route not in ('fused', 'composed'):
                raise ValueError(f"route must be 'fused' or 'composed', got {route!r}")
            self.route = route
        self.last_best_index = None

    def weights(self):
        return (self.global_pred_trimap_ce_loss_weight, self.global_pred_trimap_iou_loss_weight, self.local_pred_alpha_loss_weight,
                self.local_pred_laplacian_loss_weight, self.fusion_pred_alpha_loss_weight, self.fusion_pred_laplacian_loss_weight,
                self.composition_loss_weight, self.iou_predict_loss_weight)

    def forward(self, images, inputs, targets):
        all_global, all_local, all_fused, all_iou = inputs
        masks, trimaps, fg_maps, bg_maps = targets
        assert len(all_global) == len(all_local) == len(all_fused) == len(all_iou)
        iter_num = len(all_global)
        totals = [0.] * 8
        for gp, lp, fp, ip in zip(all_global, all_local, all_fused, all_iou):
            for i, v in enumerate(self.compute_per_iter_matting_loss(gp, lp, fp, ip, images, masks, trimaps, fg_maps, bg_maps)):
                totals[i] = totals[i] + v
        return {k: wgt * (v / float(iter_num)) for k, wgt, v in zip(LOSS_KEYS, self.weights(), totals)}

    def tables(self, global_preds, local_preds, fused_preds, iou_preds, images, masks, trimaps, fg_maps, bg_maps):
        """-> the eight [B, M] tables, divided by B as the reference's compute_* methods leave them"""
        fn = fused_tables if (global_preds.is_cuda and self.route == 'fused') else composed_tables
        dev = global_preds.device
        images, masks, trimaps, fg_maps, bg_maps = (t.to(dev) for t in (images, masks, trimaps, fg_maps, bg_maps))
        tabs = fn(global_preds, local_preds, fused_preds, iou_preds, images, masks, trimaps, fg_maps, bg_maps, self.mask_threshold)
        batch = global_preds.shape[0]
        return [t / batch for t in tabs]

    def compute_per_iter_matting_loss(self, per_iter_global_preds, per_iter_local_preds, per_iter_fused_preds, per_iter_iou_preds,
                                      images, masks, trimaps, fg_maps, bg_maps):
        tabs = self.tables(per_iter_global_preds, per_iter_local_preds, per_iter_fused_preds, per_iter_iou_preds, images, masks,
                           trimaps, fg_maps, bg_maps)
        if self.reduce_all_masks:
            return [t.mean(dim=-1, keepdim=True).sum() for t in tabs]
        if tabs[0].shape[1] > 1:
            combine = 0.
            for t, wgt in zip(tabs[:7], self.weights()[:7]):
                combine = combine + t * wgt
            best = torch.argmin(combine, dim=-1, keepdim=True)
            self.last_best_index = best.detach().squeeze(1)
            kept = [torch.gather(t, 1, best) for t in tabs[:7]]
            kept.append(tabs[7].mean(dim=-1, keepdim=True) if self.supervise_all_iou else torch.gather(tabs[7], 1, best))
            tabs = kept
        return [t.sum() for t in tabs]


class SAMMattingMultiLevelLoss(SAMMattingLoss):
    reduce_all_masks = True

    def __init__(self,
                 global_pred_trimap_ce_loss_weight=1,
                 global_pred_trimap_iou_loss_weight=1,
                 local_pred_alpha_loss_weight=1,
                 local_pred_laplacian_loss_weight=1,
                 fusion_pred_alpha_loss_weight=1,
                 fusion_pred_laplacian_loss_weight=1,
                 composition_loss_weight=1,
                 iou_predict_loss_weight=1,
                 mask_threshold=0.5,
                 route=None):
        super(SAMMattingMultiLevelLoss, self).__init__(
            global_pred_trimap_ce_loss_weight=global_pred_trimap_ce_loss_weight,
            global_pred_trimap_iou_loss_weight=global_pred_trimap_iou_loss_weight,
            local_pred_alpha_loss_weight=local_pred_alpha_loss_weight,
            local_pred_laplacian_loss_weight=local_pred_laplacian_loss_weight,
            fusion_pred_alpha_loss_weight=fusion_pred_alpha_loss_weight,
            fusion_pred_laplacian_loss_weight=fusion_pred_laplacian_loss_weight,
            composition_loss_weight=composition_loss_weight,
            iou_predict_loss_weight=iou_predict_loss_weight,
            supervise_all_iou=True,
            mask_threshold=mask_threshold,
            route=route)
