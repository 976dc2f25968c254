"""Losses of the reference's human-matting family (SimpleAICV/human_matting/losses.py): same class names (`GloabelTrimapIouLoss`
as the reference spells it), constructor arguments and call signatures.

On device tensors every loss reads the full-resolution fp32 maps through csrc/matting.hip: a few per-sample sums in one pass
(`ops.trimap_stats`, `ops.alpha_l1`, `ops.composition_l1`) or one launch per pyramid level (`ops.laplacian_l1`, ONE pyramid of
(clamp(pred) - alpha) * w instead of the reference's two -- the pyramid is linear), one pass back from gradients that stay on
the device, and the rest is a few [B]-sized torch ops: a captured step can hold all seven.  All sums are ordered: the losses are
bit-reproducible in every mode.

On CPU tensors the same classes run the reference formulas as torch ops (host tests, float64 judges).  Every class also carries
`route`: 'fused' (the kernels, the default on device tensors) or 'composed' (the reference formula as torch ops on the device too).
A fused route is the default only where scripts/probes/matting_bench.py measured it faster than the composed one on the same GPU
(profiles/matting_step.json); the composed route stays selectable per instance: `loss.route = 'composed'`."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops

__all__ = [
    'GlobalTrimapCELoss',
    'GloabelTrimapIouLoss',
    'LocalAlphaLoss',
    'LocalLaplacianLoss',
    'FusionAlphaLoss',
    'FusionLaplacianLoss',
    'CompositionLoss',
]


def _trimap_one_hot(global_pred, trimap):
    """the reference's preamble of both trimap losses -> clamped predictions [N, 3] and the one-hot labels [N, 3]"""
    global_pred = global_pred.float().permute(0, 2, 3, 1).contiguous()
    num_classes = global_pred.shape[3]
    global_pred = torch.clamp(global_pred, min=1e-4, max=1. - 1e-4)
    convert_trimap = trimap.clone()
    convert_trimap[convert_trimap == 0] = 0
    convert_trimap[convert_trimap == 255] = 2
    convert_trimap[convert_trimap > 2] = 1
    return global_pred.view(-1, num_classes), F.one_hot(convert_trimap.view(-1).long(), num_classes=num_classes).float()


class GlobalTrimapCELoss(nn.Module):
    route = 'fused'

    def __init__(self):
        super(GlobalTrimapCELoss, self).__init__()

    def forward(self, global_pred, trimap):
        if global_pred.is_cuda and self.route == 'fused':
            return ops.trimap_stats(global_pred, trimap)[:, 0].sum() / float(global_pred.numel())
        pred, label = _trimap_one_hot(global_pred, trimap)
        return (-(label * torch.log(pred) + (1. - label) * torch.log(1. - pred))).mean()


class GloabelTrimapIouLoss(nn.Module):
    route = 'fused'

    def __init__(self, smooth=1e-4):
        super(GloabelTrimapIouLoss, self).__init__()
        self.smooth = smooth

    def forward(self, global_pred, trimap):
        if global_pred.is_cuda and self.route == 'fused':
            return ops.trimap_stats(global_pred, trimap, self.smooth)[:, 1].sum() / float(global_pred.numel() // 3)
        pred, label = _trimap_one_hot(global_pred, trimap)
        intersection = pred * label
        iou_loss = 1. - (torch.sum(intersection, dim=1) + self.smooth) / (
            torch.sum(pred, dim=1) + torch.sum(label, dim=1) - torch.sum(intersection, dim=1) + self.smooth)
        return iou_loss.mean()


def _alpha_reference(pred, alpha, weighted):
    pred = torch.clamp(pred.float().permute(0, 2, 3, 1).contiguous(), min=1e-4, max=1. - 1e-4)
    diff = torch.squeeze(pred, dim=-1) - alpha
    return torch.sqrt((diff if weighted is None else diff * weighted) ** 2 + 1e-12)


class LocalAlphaLoss(nn.Module):
    route = 'fused'

    def __init__(self):
        super(LocalAlphaLoss, self).__init__()

    def forward(self, local_pred, alpha, trimap):
        if local_pred.is_cuda and self.route == 'fused':
            return ops.alpha_loss(local_pred, alpha, trimap)
        weighted = torch.zeros_like(trimap)
        weighted[trimap == 128] = 1.
        return _alpha_reference(local_pred, alpha, weighted).sum() / (weighted.sum() + 1.)


class FusionAlphaLoss(nn.Module):
    route = 'fused'

    def __init__(self):
        super(FusionAlphaLoss, self).__init__()

    def forward(self, fusion_pred, alpha):
        if fusion_pred.is_cuda and self.route == 'fused':
            return ops.alpha_loss(fusion_pred, alpha)
        return _alpha_reference(fusion_pred, alpha, None).sum() / torch.ones_like(alpha).sum()


class _LaplacianLoss(nn.Module):
    """the reference's pyramid code, shared by the two Laplacian losses (it repeats it in both classes)"""
    route = 'fused'

    def build_gauss_kernel(self, size=5, sigma=1.0, n_channels=1):
        if size % 2 != 1:
            raise ValueError("kernel size must be uneven")
        grid = np.float32(np.mgrid[0:size, 0:size].T)
        kernel = np.sum(np.exp(-((grid - size // 2) ** 2) / (2 * sigma ** 2)), axis=2)
        kernel /= np.sum(kernel)
        kernel = np.tile(kernel, (n_channels, 1, 1))
        return torch.FloatTensor(kernel[:, None, :, :])

    def laplacian_pyramid(self, img, kernel, max_levels=5):
        current, pyr = img, []
        for _ in range(max_levels):
            filtered = self.conv_gauss(current, kernel)
            pyr.append(current - filtered)
            current = F.avg_pool2d(filtered, 2)
        pyr.append(current)
        return pyr

    def conv_gauss(self, img, kernel):
        n_channels, _, kw, kh = kernel.shape
        img = F.pad(img, (kw // 2, kh // 2, kw // 2, kh // 2), mode='replicate')
        return F.conv2d(img, kernel, groups=n_channels)

    def _reference(self, pred, alpha, weighted):
        pred = torch.clamp(pred.float(), min=1e-4, max=1. - 1e-4)
        alpha = torch.unsqueeze(alpha, dim=1)
        if weighted is not None:
            pred, alpha = pred * weighted, alpha * weighted
        kernel = self.build_gauss_kernel(size=5, sigma=1.0, n_channels=1).to(pred.device)
        return sum(F.l1_loss(a, b) for a, b in zip(self.laplacian_pyramid(alpha, kernel, 5), self.laplacian_pyramid(pred, kernel, 5)))


class LocalLaplacianLoss(_LaplacianLoss):

    def __init__(self):
        super(LocalLaplacianLoss, self).__init__()

    def forward(self, local_pred, alpha, trimap):
        if local_pred.is_cuda and self.route == 'fused':
            return ops.laplacian_l1(local_pred, alpha, trimap)
        trimap = torch.unsqueeze(trimap, dim=1)
        weighted = torch.zeros_like(trimap)
        weighted[trimap == 128] = 1.
        return self._reference(local_pred, alpha, weighted)


class FusionLaplacianLoss(_LaplacianLoss):

    def __init__(self):
        super(FusionLaplacianLoss, self).__init__()

    def forward(self, fusion_pred, alpha):
        if fusion_pred.is_cuda and self.route == 'fused':
            return ops.laplacian_l1(fusion_pred, alpha)
        return self._reference(fusion_pred, alpha, None)


class CompositionLoss(nn.Module):
    route = 'fused'

    def __init__(self):
        super(CompositionLoss, self).__init__()

    def forward(self, image, alpha, fg_map, bg_map, fusion_pred):
        if fusion_pred.is_cuda and self.route == 'fused':
            return ops.composition_l1(fusion_pred, fg_map, bg_map, image).sum() / float(alpha.numel())
        fusion_pred = torch.clamp(fusion_pred.float(), min=1e-4, max=1. - 1e-4)
        fusion_pred = torch.cat([fusion_pred, fusion_pred, fusion_pred], dim=1)
        composition = fusion_pred * fg_map + (1. - fusion_pred) * bg_map
        return torch.sqrt((composition - image) ** 2 + 1e-12).sum() / torch.ones_like(alpha).sum()
