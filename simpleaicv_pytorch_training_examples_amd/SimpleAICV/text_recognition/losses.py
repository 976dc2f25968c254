"""Losses of the reference's text-recognition family (SimpleAICV/text_recognition/losses.py): same names, constructor arguments
and call signatures.

CTCLoss(preds [T, B, C], trans_targets [B, str_max_length], input_lengths [B], target_lengths [B]) -> scalar.  On device tensors
with `route = 'fused'` it is `ops.ctc_loss` (csrc/ctc.hip): the logits stay in their dtype and strides (the permuted view of the
model's [B, T, C] output is read as it is), no fp32 copy and no log-softmax tensor exist, all sums are ordered (bit-reproducible in
every mode; torch's GPU CTC backward is not), and nothing is read back to the host.  `route = 'composed'` runs the reference
formula as torch ops on the device; on CPU tensors every instance does (host tests, float64 judges).  The per-sample negative
log-likelihoods of the last call are kept in `last_nll` (detached).

Differences from the reference on the fused route: entries of trans_targets at or beyond a sample's target length are never
looked at; a sample with a label outside [0, C) or equal to the blank is dropped like an infeasible one (torch raises or reads out of
bounds).

ACELoss is the reference's formula as torch ops on any device: the per-sample class histogram is one scatter_add on the device
instead of the reference's host loop over a numpy copy.  No reference config uses it, so it has no kernel."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops

__all__ = [
    'CTCLoss',
    'ACELoss',
]


class CTCLoss(nn.Module):
    route = 'fused'

    def __init__(self, blank_index, use_focal_weight=False, gamma=2.0):
        super(CTCLoss, self).__init__()
        self.blank_index = blank_index
        self.use_focal_weight = use_focal_weight
        self.gamma = gamma
        self.last_nll = None

    def forward(self, preds, trans_targets, input_lengths, target_lengths):
        if preds.is_cuda and self.route == 'fused':
            dev = preds.device
            loss, self.last_nll = ops.ctc_loss(preds, trans_targets.to(dev), input_lengths.to(dev), target_lengths.to(dev),
                                               self.blank_index, self.gamma if self.use_focal_weight else None)
            return loss
        preds = preds.float()
        dev = preds.device
        trans_targets, input_lengths, target_lengths = trans_targets.to(dev), input_lengths.to(dev), target_lengths.to(dev)
        batch = preds.shape[1]
        preds = F.log_softmax(preds, dim=2)
        loss = F.ctc_loss(preds, trans_targets.long(), input_lengths.long(), target_lengths.long(), blank=self.blank_index,
                          reduction='none', zero_infinity=True)
        self.last_nll = loss.detach()
        if self.use_focal_weight:
            pt = torch.exp(-loss)
            loss = torch.pow((1. - pt), self.gamma) * loss
        return (loss / target_lengths / batch).sum()


class ACELoss(nn.Module):

    def __init__(self, blank_index=0):
        super(ACELoss, self).__init__()
        self.blank_index = blank_index

    def __call__(self, preds, trans_targets):
        preds = preds.float()
        t, b, num_classes = preds.shape
        preds = F.softmax(preds, dim=2).mean(dim=0)
        tg = trans_targets.to(preds.device).long()
        keep = tg < num_classes                                             # (the garbage index num_classes + 1 ... is dropped)
        counts = torch.zeros((b, num_classes), dtype=torch.float32, device=preds.device)
        counts.scatter_add_(1, tg.clamp(max=num_classes - 1), keep.float())
        length = (keep & (tg > 0)).sum(dim=1).float()                       # the reference's np.sum(per_trans_target > 0)
        col = torch.arange(num_classes, device=preds.device).unsqueeze(0) == self.blank_index
        counts = torch.where(col, (t - length).unsqueeze(1), counts) / t
        return (-torch.sum(torch.log(preds) * counts)) / b
