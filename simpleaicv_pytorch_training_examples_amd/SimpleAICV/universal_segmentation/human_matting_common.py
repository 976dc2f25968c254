"""Collaters of the universal-matting human-matting task (reference SimpleAICV/universal_segmentation/human_matting_common.py:
HumanMattingTestCollater :242, HumanMattingTrainCollater :311) and the transforms the synthetic dataset needs (RandomHorizontalFlip
:109, Normalize :220; the OpenCV crops and resizes are not ported: the synthetic samples are made at their final size).

A sample is {'image': float32 HWC, 'mask': the alpha matte [H, W] in [0, 1], 'trimap': uint8 [H, W] in {0, 128, 255}, 'fg_map',
'bg_map': float32 HWC, 'size', 'origin_size'}.  The train collater makes every image a list of ONE object (a human matting sample
holds one portrait, label 0) padded to resize x resize; an empty matte raises, as the reference's assert does."""
import numpy as np
import torch

from ..classification.common import load_state_dict  # noqa: F401  (re-exported, as in the reference)


class RandomHorizontalFlip:

    def __init__(self, prob=0.5):
        self.prob = prob

    def __call__(self, sample):
        if np.random.uniform(0, 1) < self.prob:
            for key in ('image', 'fg_map', 'bg_map'):
                sample[key] = sample[key][:, ::-1, :]
            for key in ('mask', 'trimap'):
                sample[key] = sample[key][:, ::-1]
        return sample


class Normalize:

    def __call__(self, sample):
        for key in ('image', 'fg_map', 'bg_map'):
            sample[key] = sample[key] / 255.
        return sample


def _pad(maps, resize, dtype=np.float32):
    """a list of [h, w] or [h, w, 3] arrays -> float tensor [N, resize, resize] or [N, 3, resize, resize], zero padded"""
    out = np.zeros((len(maps), resize, resize) + tuple(maps[0].shape[2:]), dtype=dtype)
    for i, m in enumerate(maps):
        out[i, 0:m.shape[0], 0:m.shape[1]] = m
    out = torch.from_numpy(out)
    return (out.permute(0, 3, 1, 2) if out.dim() == 4 else out).float()


class HumanMattingTestCollater:

    def __init__(self, resize=1024):
        self.resize = resize

    def __call__(self, data):
        return {
            'image': _pad([s['image'] for s in data], self.resize),
            'mask': _pad([s['mask'] for s in data], self.resize),
            'trimap': _pad([s['trimap'] for s in data], self.resize, np.uint8),
            'fg_map': _pad([s['fg_map'] for s in data], self.resize),
            'bg_map': _pad([s['bg_map'] for s in data], self.resize),
            'size': np.array([s['size'] for s in data], dtype=np.float32),
            'origin_size': np.array([s['origin_size'] for s in data], dtype=np.float32),
        }


class HumanMattingTrainCollater:

    def __init__(self, resize=1024):
        self.resize = resize

    def __call__(self, data):
        masks, trimaps, fg_maps, bg_maps, labels = [], [], [], [], []
        for s in data:
            assert np.count_nonzero(s['mask']) > 0                      # every image holds a portrait
            masks.append(_pad([s['mask']], self.resize))
            trimaps.append(_pad([s['trimap']], self.resize, np.uint8))
            fg_maps.append(_pad([s['fg_map']], self.resize))
            bg_maps.append(_pad([s['bg_map']], self.resize))
            labels.append(torch.zeros(1, dtype=torch.int64))            # one portrait per image, class 0
        return {
            'image': _pad([s['image'] for s in data], self.resize),
            'mask': masks,
            'trimap': trimaps,
            'fg_map': fg_maps,
            'bg_map': bg_maps,
            'label': labels,
            'size': np.array([s['size'] for s in data], dtype=np.float32),
        }
