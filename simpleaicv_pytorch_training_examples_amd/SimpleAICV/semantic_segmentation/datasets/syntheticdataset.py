"""Synthetic stand-in for the reference's ADE20KSemanticSegmentation / CocoSemanticSegmentation datasets + transform block in the
benchmark configs: a sample has the contract the reference hands to SemanticSegmentationCollater AFTER its transforms
(semantic_segmentation/common.py:109-143): {'image': float32 HWC (normalised), 'mask': float32 HW class ids (0 = background),
'size': [h, w]}.  The mask is a few axis-aligned rectangles of random classes over background and the image carries each class as
a colour offset under noise, so a network can learn the mapping (the training-loop test checks that the loss falls)."""
import numpy as np
from torch.utils.data import Dataset


class SyntheticSemanticSegmentationDataset(Dataset):

    def __init__(self, num_samples, height, width, num_classes=151, max_regions=6, seed=0):
        self.num_samples, self.height, self.width = num_samples, height, width
        self.num_classes, self.max_regions, self.seed = num_classes, max_regions, seed
        self.palette = np.random.default_rng(seed).uniform(-2., 2., (num_classes, 3)).astype(np.float32)

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx):
        rng = np.random.default_rng((self.seed, idx))
        h, w = self.height, self.width
        mask = np.zeros((h, w), dtype=np.float32)
        for _ in range(int(rng.integers(1, self.max_regions + 1))):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            y1, x1 = min(h, y0 + int(rng.integers(h // 8 + 1, h // 2 + 2))), min(w, x0 + int(rng.integers(w // 8 + 1, w // 2 + 2)))
            mask[y0:y1, x0:x1] = float(rng.integers(1, self.num_classes))
        image = self.palette[mask.astype(np.int64)] + 0.5 * rng.standard_normal((h, w, 3), dtype=np.float32)
        return {'image': image.astype(np.float32), 'mask': mask, 'size': np.array([h, w], dtype=np.float32)}
