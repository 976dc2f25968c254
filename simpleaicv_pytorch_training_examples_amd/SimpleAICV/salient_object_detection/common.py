"""Batch collater of the salient-object-detection pipeline -- drop-in for the reference SalientObjectDetectionSegmentationCollater
(SimpleAICV/salient_object_detection/common.py:191-223): images at the top-left of a zero [B, S, S, 3] canvas handed over as its
NCHW view (channels-last memory, what the convolution kernels stream), masks [B, S, S] float32 in [0, 1] padded with 0, sizes
[B, 2] float32 (numpy).  The reference's OpenCV transforms (YoloStyleResize, Resize, RandomHorizontalFlip, Normalize) are not part
of the benchmark pipeline, whose synthetic dataset delivers samples as they leave those transforms."""
import numpy as np
import torch

from ..classification.common import load_state_dict  # noqa: F401  (re-exported, as in the reference)


class SalientObjectDetectionSegmentationCollater:

    def __init__(self, resize=1024):
        self.resize = resize

    def __call__(self, data):
        n, s = len(data), self.resize
        canvas = np.zeros((n, s, s, 3), dtype=np.float32)
        masks = np.zeros((n, s, s), dtype=np.float32)
        for i, sample in enumerate(data):
            image, mask = sample['image'], sample['mask']
            canvas[i, 0:image.shape[0], 0:image.shape[1], :] = image
            masks[i, 0:mask.shape[0], 0:mask.shape[1]] = mask
        return {
            'image': torch.from_numpy(canvas).permute(0, 3, 1, 2).float(),        # B H W 3 -> B 3 H W (view)
            'mask': torch.from_numpy(masks).float(),
            'size': np.array([x['size'] for x in data], dtype=np.float32),
        }
