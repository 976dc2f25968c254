"""Losses of the reference's salient-object-detection family (SimpleAICV/salient_object_detection/losses.py): same class names,
constructor arguments and call signature `loss(pred [B, 1, H, W] probabilities, label [B, H, W] soft mask in [0, 1]) -> scalar`.

BCELoss (:16-38), BCEIouloss (:80-106) and BCEDiceLoss (:109-134) each read the full-resolution maps only through four sums per
sample -- sum bce, sum ph, sum l, sum ph * l over ph = clamp(pred, 1e-4, 1 - 1e-4) -- which `ops.binary_seg_stats` (csrc/salient.hip)
takes in one pass; the rest is a few [B]-sized torch ops.  Losses called on the same prediction share that pass (and its one
backward pass).  A prediction that is not fp32-contiguous is made so first, as the reference's `pred.float()` ... `.contiguous()`.

OHEMBCELoss (:41-77) is the reference formula in torch ops.  It reads two counts on the host (`int(mask.sum())`), as the reference
does, so it is eager-only: a captured step cannot contain it."""
import torch
import torch.nn as nn

from ... import ops

__all__ = [
    'BCELoss',
    'OHEMBCELoss',
    'BCEIouloss',
    'BCEDiceLoss',
]


def _stats(pred, label):
    """-> stats [B, 4] and the number of elements per sample"""
    assert pred.dim() == 4 and pred.shape[1] == 1
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        pred = pred.float().contiguous()
    return ops.binary_seg_stats(pred, label), pred[0].numel()


class BCELoss(nn.Module):

    def __init__(self):
        super(BCELoss, self).__init__()

    def forward(self, pred, label):
        stats, per_sample = _stats(pred, label)
        return stats[:, 0].sum() / float(stats.shape[0] * per_sample)


class OHEMBCELoss(nn.Module):

    def __init__(self, negative_ratio=1.5):
        super(OHEMBCELoss, self).__init__()
        self.negative_ratio = negative_ratio

    def forward(self, pred, label):
        pred = pred.float().permute(0, 2, 3, 1).contiguous()
        assert pred.shape[3] == 1
        pred = torch.clamp(pred, min=1e-4, max=1. - 1e-4).view(-1)
        label = label.reshape(-1)
        positive_point_mask = (label > 0).float()
        positive_points_num = int(positive_point_mask.sum())
        negative_points_num = min(int((1. - positive_point_mask).sum()), int(positive_points_num * self.negative_ratio))
        loss = -(label * torch.log(pred) + (1. - label) * torch.log(1. - pred))
        positive_loss = loss * positive_point_mask
        negative_loss, _ = torch.topk((loss * (1. - positive_point_mask)).view(-1), negative_points_num)
        return (positive_loss.sum() + negative_loss.sum()) / (positive_points_num + negative_points_num + 1e-4)


class BCEIouloss(nn.Module):

    def __init__(self, smooth=1e-4):
        super(BCEIouloss, self).__init__()
        self.smooth = smooth

    def forward(self, pred, label):
        stats, _ = _stats(pred, label)
        inter = stats[:, 3]
        return (1. - (inter + self.smooth) / (stats[:, 1] + stats[:, 2] - inter + self.smooth)).mean()


class BCEDiceLoss(nn.Module):

    def __init__(self, smooth=1e-4):
        super(BCEDiceLoss, self).__init__()
        self.smooth = smooth

    def forward(self, pred, label):
        stats, _ = _stats(pred, label)
        return (1. - (2 * stats[:, 3] + self.smooth) / (stats[:, 1] + stats[:, 2] + self.smooth)).mean()
