"""Host-side sample transforms and the batch collater of the SAM matting pipeline -- drop-in for the reference
(SimpleAICV/interactive_segmentation/common_matting.py): SAMMattingResize (:278), SAMMattingRandomHorizontalFlip (:361),
SAMMattingNormalize (:473), SAMMattingBatchCollater (:509-652), load_state_dict.

A sample carries the SAM keys (image float32 HWC, box, mask -- here a SOFT alpha in [0, 1] --, size, prompt_point [P, 3], prompt_box,
prompt_mask) and trimap (uint8 0 / 128 / 255), fg_map, bg_map (HWC, normalised like the image).  The collater pads every map with
zeros to the square canvas at the top-left and gives ten keys: image [B, 3, S, S], box [B, 4], mask [B, 1, S, S], size (numpy
[B, 2]), prompt_point [B, P, 3], prompt_box [B, 4], prompt_mask [B, 1, S / 4, S / 4], trimap [B, S, S], fg_map and bg_map
[B, 3, S, S]; all fp32.

OpenCV is optional: the collater's bilinear resize of the prompt mask is numpy with OpenCV's INTER_LINEAR sampling rule (source
coordinate (dst + 0.5) * scale - 0.5, clamped; no antialiasing), SAMMattingResize's image resampling needs cv2 and imports it when
called.  The reference's random scale / translate / gray / vertical-flip augmentations warp with OpenCV throughout and are not
ported."""
import numpy as np
import torch

from ..classification.common import load_state_dict  # noqa: F401  (re-exported, as in the reference)
from .common import resize_nearest


def resize_linear(arr, width, height):
    """cv2.resize(arr, (width, height)) (INTER_LINEAR) for 2-d float arrays"""
    h, w = arr.shape[:2]
    if (h, w) == (height, width):
        return arr

    def taps(n_dst, n_src):
        pos = (np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5
        i0 = np.floor(pos).astype(np.int64)
        frac = (pos - i0).astype(np.float32)
        return np.clip(i0, 0, n_src - 1), np.clip(i0 + 1, 0, n_src - 1), frac

    y0, y1, fy = taps(height, h)
    x0, x1, fx = taps(width, w)
    arr = arr.astype(np.float32)
    top = arr[y0][:, x0] * (1. - fx) + arr[y0][:, x1] * fx
    bot = arr[y1][:, x0] * (1. - fx) + arr[y1][:, x1] * fx
    return top * (1. - fy)[:, None] + bot * fy[:, None]


class SAMMattingResize:

    def __init__(self, resize=1024):
        self.resize = resize

    def __call__(self, sample):
        import cv2   # bilinear resampling of the colour maps; not needed by the synthetic generators
        image = sample['image']
        h, w, _ = image.shape
        factor = self.resize / max(h, w)
        resize_h, resize_w = int(round(h * factor)), int(round(w * factor))
        sample['image'] = cv2.resize(image, (resize_w, resize_h))
        sample['box'][0:4] *= factor
        sample['mask'] = cv2.resize(sample['mask'], (resize_w, resize_h))
        sample['size'] = np.array([resize_h, resize_w]).astype(np.float32)
        sample['prompt_point'][:, 0:2] *= factor
        sample['prompt_box'][0:4] *= factor
        sample['prompt_mask'] = cv2.resize(sample['prompt_mask'], (resize_w, resize_h))
        sample['trimap'] = resize_nearest(sample['trimap'], resize_w, resize_h)
        sample['fg_map'] = cv2.resize(sample['fg_map'], (resize_w, resize_h))
        sample['bg_map'] = cv2.resize(sample['bg_map'], (resize_w, resize_h))
        return sample


class SAMMattingRandomHorizontalFlip:

    def __init__(self, prob=0.5):
        self.prob = prob

    def __call__(self, sample):
        if np.random.uniform(0, 1) < self.prob:
            box, prompt_box, prompt_point = sample['box'], sample['prompt_box'], sample['prompt_point']
            for k in ('image', 'fg_map', 'bg_map'):
                sample[k] = sample[k][:, ::-1, :]
            for k in ('mask', 'trimap', 'prompt_mask'):
                sample[k] = sample[k][:, ::-1]
            w = sample['image'].shape[1]
            x1, x2 = box[0].copy(), box[2].copy()
            box[0], box[2] = w - x2, w - x1
            x1, x2 = prompt_box[0].copy(), prompt_box[2].copy()
            prompt_box[0], prompt_box[2] = w - x2, w - x1
            for i in range(len(prompt_point)):
                prompt_point[i][0] = w - prompt_point[i][0]
        return sample


class SAMMattingNormalize:

    def __init__(self, mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]):
        self.mean = np.expand_dims(np.expand_dims(np.array(mean), axis=0), axis=0)
        self.std = np.expand_dims(np.expand_dims(np.array(std), axis=0), axis=0)

    def __call__(self, sample):
        for k in ('image', 'fg_map', 'bg_map'):
            sample[k] = (sample[k] - self.mean) / self.std
        return sample


class SAMMattingBatchCollater:

    def __init__(self, resize):
        self.resize = resize
        assert resize % 64 == 0
        self.prompt_mask_size = resize // 4

    def _canvas(self, maps, channels, dtype=np.float32):
        s = self.resize
        out = np.zeros((len(maps), s, s) + ((channels,) if channels else ()), dtype=dtype)
        for i, m in enumerate(maps):
            out[i, 0:m.shape[0], 0:m.shape[1]] = m
        return torch.from_numpy(out)

    def __call__(self, data):
        boxes = np.zeros((len(data), 4), dtype=np.float32)
        prompt_boxes = np.zeros((len(data), 4), dtype=np.float32)
        for i, x in enumerate(data):
            boxes[i, 0:x['box'].shape[0]] = x['box'][0:4]
            prompt_boxes[i, 0:x['prompt_box'].shape[0]] = x['prompt_box'][0:4]
        prompt_masks = []
        for x in data:
            pm = x['prompt_mask']
            h, w = pm.shape
            factor = self.prompt_mask_size / max(h, w)
            pm = resize_linear(pm, int(round(w * factor)), int(round(h * factor)))
            canvas = np.zeros((self.prompt_mask_size, self.prompt_mask_size), dtype=np.float32)
            canvas[0:pm.shape[0], 0:pm.shape[1]] = pm
            prompt_masks.append(torch.from_numpy(canvas))
        return {
            'image': self._canvas([x['image'] for x in data], 3).permute(0, 3, 1, 2).contiguous().float(),
            'box': torch.from_numpy(boxes).float(),
            'mask': self._canvas([x['mask'] for x in data], 0).unsqueeze(1).float(),
            'size': np.array([x['size'] for x in data], dtype=np.float32),
            'prompt_point': torch.stack([torch.from_numpy(x['prompt_point']) for x in data], dim=0).float(),
            'prompt_box': torch.from_numpy(prompt_boxes).float(),
            'prompt_mask': torch.stack(prompt_masks, dim=0).unsqueeze(1).float(),
            'trimap': self._canvas([x['trimap'] for x in data], 0, np.uint8).float(),
            'fg_map': self._canvas([x['fg_map'] for x in data], 3).permute(0, 3, 1, 2).float(),
            'bg_map': self._canvas([x['bg_map'] for x in data], 3).permute(0, 3, 1, 2).float(),
        }
