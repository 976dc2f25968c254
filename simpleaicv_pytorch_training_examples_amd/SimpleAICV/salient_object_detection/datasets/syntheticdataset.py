"""Synthetic stand-in for the reference's SalientObjectDetectionDataset + transform block in the benchmark configs: a sample has the
contract the reference hands to SalientObjectDetectionSegmentationCollater AFTER its transforms
(salient_object_detection/common.py:191-223): {'image': float32 HWC (normalised), 'mask': float32 HW in [0, 1], 'size': [h, w]}.
The mask is one or two soft-edged ellipses (1 inside, a linear ramp over a few pixels, 0 outside -- the reference's masks are
anti-aliased alpha mattes divided by 255) and the image carries the mask as a colour offset under noise, so a network can learn the
mapping (the training-loop test checks that the loss falls)."""
import numpy as np
from torch.utils.data import Dataset


class SyntheticSalientObjectDetectionDataset(Dataset):

    def __init__(self, num_samples, height, width, max_objects=2, seed=0):
        self.num_samples, self.height, self.width = num_samples, height, width
        self.max_objects, self.seed = max_objects, seed
        self.colour = np.random.default_rng(seed).uniform(1., 2., 3).astype(np.float32)

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx):
        rng = np.random.default_rng((self.seed, idx))
        h, w = self.height, self.width
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        mask = np.zeros((h, w), dtype=np.float32)
        for _ in range(int(rng.integers(1, self.max_objects + 1))):
            cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
            ry, rx = rng.uniform(0.12, 0.35) * h, rng.uniform(0.12, 0.35) * w
            d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
            edge = 3. / min(ry, rx)                                                # a ramp about three pixels wide
            mask = np.maximum(mask, np.clip((1. + edge - d) / (2. * edge), 0., 1.).astype(np.float32))
        image = mask[:, :, None] * self.colour + 0.5 * rng.standard_normal((h, w, 3), dtype=np.float32)
        return {'image': image.astype(np.float32), 'mask': mask, 'size': np.array([h, w], dtype=np.float32)}
