"""UniversalMattingDecoder -- drop-in for the reference's SimpleAICV/universal_segmentation/matting_decode.py (:19): per image the
fused alpha mattes of the queries whose best foreground class scores above min_score_threshold, sorted by score, at most topk,
cropped to the scaled size and resized bilinearly to the original size; numpy outputs.  (An image that keeps nothing gets an empty
[0, H, W] array of the prediction's size.)"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = [
    'UniversalMattingDecoder',
]


class UniversalMattingDecoder(nn.Module):

    def __init__(self, topk=100, min_score_threshold=0.1):
        super(UniversalMattingDecoder, self).__init__()
        self.topk = topk
        self.min_score_threshold = min_score_threshold

    @torch.no_grad()
    def forward(self, preds, scaled_sizes, origin_sizes):
        _, _, fused_preds, class_preds = preds
        h, w = fused_preds.shape[-2], fused_preds.shape[-1]
        # the last class is the background: what no kept query claims is background
        scores, classes = torch.max(torch.softmax(class_preds.float(), dim=-1)[:, :, :-1], dim=-1)
        batch_masks, batch_scores, batch_classes = [], [], []
        for fused, score, cls, scaled, origin in zip(fused_preds, scores, classes, scaled_sizes, origin_sizes):
            keep = torch.nonzero(score > self.min_score_threshold).flatten()
            keep = keep[torch.argsort(score[keep], descending=True)][:self.topk]
            if keep.numel() == 0:
                batch_masks.append(np.zeros((0, h, w), dtype=np.float32))
                batch_scores.append(np.zeros((0, ), dtype=np.float32))
                batch_classes.append(np.zeros((0, ), dtype=np.float32))
                continue
            mattes = fused[keep, 0, :int(scaled[0]), :int(scaled[1])].float()
            mattes = F.interpolate(mattes.unsqueeze(0), size=[int(origin[0]), int(origin[1])], mode='bilinear').squeeze(0)
            batch_masks.append(mattes.cpu().numpy())
            batch_scores.append(score[keep].cpu().numpy())
            batch_classes.append(cls[keep].cpu().numpy())
        return batch_masks, batch_scores, batch_classes
