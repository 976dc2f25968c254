"""Batch collater of the human-matting pipeline -- drop-in for the reference HumanMattingCollater
(SimpleAICV/human_matting/common.py:236-299): image, fg_map and bg_map at the top-left of zero [B, S, S, 3] canvases handed over as
their NCHW views (channels-last memory, what the convolution kernels stream), mask [B, S, S] float32 in [0, 1] and trimap [B, S, S]
(uint8 values 0 / 128 / 255 as float32) padded with 0, sizes [B, 2] float32 (numpy).  The reference's OpenCV transforms
(YoloStyleResize, Resize, RandomHorizontalFlip, Normalize) are not part of the benchmark pipeline, whose synthetic dataset delivers
samples as they leave those transforms."""
import numpy as np
import torch

from ..classification.common import load_state_dict  # noqa: F401  (re-exported, as in the reference)


class HumanMattingCollater:

    def __init__(self, resize=1024):
        self.resize = resize

    def __call__(self, data):
        n, s = len(data), self.resize

        def canvas3(key):
            out = np.zeros((n, s, s, 3), dtype=np.float32)
            for i, sample in enumerate(data):
                v = sample[key]
                out[i, 0:v.shape[0], 0:v.shape[1], :] = v
            return torch.from_numpy(out).permute(0, 3, 1, 2).float()               # B H W 3 -> B 3 H W (view)

        def canvas1(key, dtype):
            out = np.zeros((n, s, s), dtype=dtype)
            for i, sample in enumerate(data):
                v = sample[key]
                out[i, 0:v.shape[0], 0:v.shape[1]] = v
            return torch.from_numpy(out).float()

        return {
            'image': canvas3('image'),
            'mask': canvas1('mask', np.float32),
            'trimap': canvas1('trimap', np.uint8),
            'fg_map': canvas3('fg_map'),
            'bg_map': canvas3('bg_map'),
            'size': np.array([x['size'] for x in data], dtype=np.float32),
        }
