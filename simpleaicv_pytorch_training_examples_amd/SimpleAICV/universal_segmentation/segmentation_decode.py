"""UniversalSegmentationDecoder (reference SimpleAICV/universal_segmentation/segmentation_decode.py:19): per image the queries whose
best foreground class probability exceeds min_score_threshold, sorted by it and cut to topk; their sigmoid masks cropped to the
scaled size, resized to the original size and (binary_mask) thresholded.  Post-processing on a few masks: torch ops."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = [
    'UniversalSegmentationDecoder',
]


class UniversalSegmentationDecoder(nn.Module):

    def __init__(self, topk=100, min_score_threshold=0.1, mask_threshold=0.5, binary_mask=True):
        super(UniversalSegmentationDecoder, self).__init__()
        self.topk = topk
        self.min_score_threshold = min_score_threshold
        self.mask_threshold = mask_threshold
        self.binary_mask = binary_mask

    @torch.no_grad()
    def forward(self, preds, scaled_sizes, origin_sizes):
        mask_preds, class_preds = preds
        h, w = mask_preds.shape[2], mask_preds.shape[3]
        mask_preds = torch.sigmoid(mask_preds.float())
        # the last class is the background: what no kept query claims is background
        pred_scores, pred_classes = torch.max(torch.softmax(class_preds.float(), dim=-1)[:, :, :-1], dim=-1)
        batch_masks, batch_scores, batch_classes = [], [], []
        for masks, scores, classes, scaled, origin in zip(mask_preds, pred_scores, pred_classes, scaled_sizes, origin_sizes):
            keep = scores > self.min_score_threshold
            masks, scores, classes = masks[keep], scores[keep], classes[keep]
            if scores.shape[0] == 0:
                batch_masks.append(np.zeros((0, h, w), dtype=np.float32))
                batch_scores.append(np.zeros((0), dtype=np.float32))
                batch_classes.append(np.zeros((0), dtype=np.float32))
                continue
            order = torch.argsort(scores, descending=True)[:self.topk]
            masks, scores, classes = masks[order], scores[order], classes[order]
            masks = masks[:, :int(scaled[0]), :int(scaled[1])]
            masks = F.interpolate(masks.unsqueeze(0), size=[int(origin[0]), int(origin[1])], mode='bilinear').squeeze(0)
            if self.binary_mask:
                masks = (masks > self.mask_threshold).to(torch.uint8)
            batch_masks.append(masks.cpu().numpy())
            batch_scores.append(scores.cpu().numpy())
            batch_classes.append(classes.cpu().numpy())
        return batch_masks, batch_scores, batch_classes
