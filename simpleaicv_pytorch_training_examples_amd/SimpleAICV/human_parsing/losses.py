"""Losses of the reference's human-parsing and face-parsing families (SimpleAICV/human_parsing/losses.py and
SimpleAICV/face_parsing/losses.py hold the same four classes): same names, constructor arguments and call signature
`loss(pred [B, C, H, W], label [B, H, W] float class ids) -> scalar`.

On device tensors every loss is one slot of `ops.pixel_class_terms` (csrc/parsing.hip): the prediction stays in its dtype and NHWC
layout, and losses over the same prediction object share ONE forward and ONE backward pass -- the reference configs train with
{CELoss, IoULoss('softmax')}.  All sums are ordered: the losses are bit-reproducible in every mode.  Difference from the
reference: a label outside [0, num_classes) contributes to no loss and no gradient (and still counts in the means); the
reference's F.one_hot raises on it.

On CPU tensors the same classes run the reference formulas as torch ops (host tests, float64 judges).  Every class also carries
`route`: 'fused' (the kernel, the default on device tensors) or 'composed' (the reference formula as torch ops on the device too),
selectable per instance: `loss.route = 'composed'`.  Fused is the default because scripts/probes/parsing_bench.py measured it
faster than both alternatives on the same GPU (profiles/parsing_step.json)."""
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


def _rows(pred, label, logit_type):
    """the reference's preamble of all four losses -> clamped probabilities [B*H*W, C] (fp32) and the one-hot labels"""
    pred = pred.float().permute(0, 2, 3, 1).contiguous()
    num_classes = pred.shape[3]
    pred = torch.softmax(pred, dim=-1) if logit_type == 'softmax' else torch.sigmoid(pred)
    pred = torch.clamp(pred, min=1e-4, max=1. - 1e-4).view(-1, num_classes)
    return pred, F.one_hot(label.reshape(-1).long(), num_classes=num_classes).float()


def _fused(loss, pred):
    return pred.is_cuda and loss.route == 'fused'


class CELoss(nn.Module):
    """mean over the pixels of -log(clamp(softmax(pred)[label], 1e-4, 1 - 1e-4))"""
    route = 'fused'

    def __init__(self):
        super(CELoss, self).__init__()

    def forward(self, pred, label):
        if _fused(self, pred):
            return ops.pixel_class_terms(pred, label, 'softmax')[0]
        pred, truth = _rows(pred, label, 'softmax')
        return ((-torch.log(pred)) * truth).sum(dim=-1).mean()


class MultiClassBCELoss(nn.Module):
    """mean over pixels and classes of the binary cross-entropy of clamp(sigmoid(pred), 1e-4, 1 - 1e-4) against the one-hot label"""
    route = 'fused'

    def __init__(self):
        super(MultiClassBCELoss, self).__init__()

    def forward(self, pred, label):
        if _fused(self, pred):
            return ops.pixel_class_terms(pred, label, 'sigmoid')[0]
        pred, truth = _rows(pred, label, 'sigmoid')
        return (-(truth * torch.log(pred) + (1. - truth) * torch.log(1. - pred))).mean()


class IoULoss(nn.Module):
    route = 'fused'

    def __init__(self, logit_type='softmax'):
        super(IoULoss, self).__init__()
        assert logit_type in ['softmax', 'sigmoid']
        self.logit_type = logit_type

    def forward(self, pred, label):
        if _fused(self, pred):
            return ops.pixel_class_terms(pred, label, self.logit_type)[1]
        pred, truth = _rows(pred, label, self.logit_type)
        inter = (pred * truth).sum(dim=1)
        union = torch.clamp(pred.sum(dim=1) + truth.sum(dim=1) - inter, min=1e-4)
        return (1. - inter / union).mean()


class DiceLoss(nn.Module):
    route = 'fused'

    def __init__(self, logit_type='softmax'):
        super(DiceLoss, self).__init__()
        assert logit_type in ['softmax', 'sigmoid']
        self.logit_type = logit_type

    def forward(self, pred, label):
        if _fused(self, pred):
            return ops.pixel_class_terms(pred, label, self.logit_type)[2]
        pred, truth = _rows(pred, label, self.logit_type)
        inter = (pred * truth).sum(dim=1)
        return (1. - (2 * inter + 1e-4) / (pred.sum(dim=1) + truth.sum(dim=1) + 1e-4)).mean()
