"""Losses of the reference's semantic-segmentation family (SimpleAICV/semantic_segmentation/losses.py): same class names,
constructor arguments and call signature `loss(pred [B, C, H, W], label [B, H, W] float class ids) -> scalar`.

CELoss (:13-43), the only loss a reference config uses, runs on the fused per-pixel kernel (`ops.pixel_softmax_ce`,
csrc/semseg.hip): the prediction stays in its dtype and NHWC layout; no fp32 copy, no permute, no one-hot tensor.  Difference
from the reference: a label outside [0, num_classes) contributes neither loss nor gradient (and still counts in the mean); the
reference's F.one_hot raises on it.

MultiClassBCELoss (:46-76), IoULoss (:79-113) and DiceLoss (:116-149) are the reference formulas written with torch ops on the
device.  No reference config uses them; they have no kernel of their own."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops

__all__ = [
    'CELoss',
    'MultiClassBCELoss',
    'IoULoss',
    'DiceLoss',
]


class CELoss(nn.Module):
    """mean over the pixels of -log(clamp(softmax(pred)[label], 1e-4, 1 - 1e-4))"""

    def __init__(self):
        super(CELoss, self).__init__()

    def forward(self, pred, label):
        return ops.pixel_softmax_ce(pred, label)


def _rows(pred, label, logit):
    """-> clamped probabilities [B*H*W, C] (fp32) and the one-hot labels of the same shape"""
    pred = pred.float().permute(0, 2, 3, 1)
    num_classes = pred.shape[3]
    pred = torch.softmax(pred, dim=-1) if logit == 'softmax' else torch.sigmoid(pred)
    pred = torch.clamp(pred, min=1e-4, max=1. - 1e-4).reshape(-1, num_classes)
    return pred, F.one_hot(label.reshape(-1).long(), num_classes=num_classes).float()


class MultiClassBCELoss(nn.Module):

    def __init__(self):
        super(MultiClassBCELoss, self).__init__()

    def forward(self, pred, label):
        pred, truth = _rows(pred, label, 'sigmoid')
        return (-(truth * torch.log(pred) + (1. - truth) * torch.log(1. - pred))).mean()


class IoULoss(nn.Module):

    def __init__(self, logit_type='softmax'):
        super(IoULoss, self).__init__()
        assert logit_type in ['softmax', 'sigmoid']
        self.logit_type = logit_type

    def forward(self, pred, label):
        pred, truth = _rows(pred, label, self.logit_type)
        inter = (pred * truth).sum(dim=1)
        union = torch.clamp(pred.sum(dim=1) + truth.sum(dim=1) - inter, min=1e-4)
        return (1. - inter / union).mean()


class DiceLoss(nn.Module):

    def __init__(self, logit_type='softmax'):
        super(DiceLoss, self).__init__()
        assert logit_type in ['softmax', 'sigmoid']
        self.logit_type = logit_type

    def forward(self, pred, label):
        pred, truth = _rows(pred, label, self.logit_type)
        inter = (pred * truth).sum(dim=1)
        return (1. - (2 * inter + 1e-4) / (pred.sum(dim=1) + truth.sum(dim=1) + 1e-4)).mean()
