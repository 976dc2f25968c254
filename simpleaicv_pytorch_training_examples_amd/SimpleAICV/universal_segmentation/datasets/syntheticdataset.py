"""Synthetic stand-in for the reference's ADE20KSemanticSegmentation + transform block (universal_segmentation/datasets/
ade20kdataset.py): a sample in the contract handed to the collaters of semantic_segmentation_common.py -- image float32 HWC in
[0, 255], mask a float32 [H, W] label map (0 = background, 1 .. num_classes - 1 foreground), size and origin_size [h, w]."""
import numpy as np
from torch.utils.data import Dataset


class SyntheticUniversalSegmentationDataset(Dataset):
    """Label maps are unions of up to max_objects axis-aligned rectangles of distinct classes over a background; the image carries
    the class as a colour offset under noise, so a model can learn it.  Every sample has at least one foreground class."""

    def __init__(self, num_samples, image_size=512, num_classes=151, max_objects=12, seed=0, transform=None):
        self.num_samples, self.image_size, self.num_classes = num_samples, image_size, num_classes
        self.max_objects, self.seed, self.transform = max_objects, seed, transform

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx):
        rng = np.random.default_rng((self.seed, idx))
        s = self.image_size
        mask = np.zeros((s, s), dtype=np.float32)
        n = int(rng.integers(1, min(self.max_objects, self.num_classes - 1) + 1))
        classes = rng.permutation(self.num_classes - 1)[:n] + 1
        for c in classes:
            y0, x0 = rng.integers(0, max(s - s // 4, 1), 2)
            hh, ww = rng.integers(max(s // 8, 1), max(s // 2, 2), 2)
            mask[y0:y0 + hh, x0:x0 + ww] = c
        image = rng.uniform(0, 96, (s, s, 3)).astype(np.float32)
        image += (mask[:, :, None] * np.array([37., 59., 83.], dtype=np.float32)) % 160.
        sample = {'image': image, 'mask': mask, 'size': np.array([s, s], dtype=np.float32),
                  'origin_size': np.array([s, s], dtype=np.float32)}
        return self.transform(sample) if self.transform is not None else sample
