"""Synthetic stand-in for the reference's HumanParsingDataset + transform block in the benchmark configs: a sample has the contract
the reference hands to HumanParsingCollater AFTER its transforms (human_parsing/common.py:317-349): {'image': float32 HWC
(normalised), 'mask': float32 HW class ids (0 = background), 'size': [h, w]}.  The mask is a few elliptical blobs of random
classes over background -- body parts are compact regions, not boxes -- and the image carries each class as a colour offset under
noise, so a network can learn the mapping (the training-loop test checks that the loss falls).  20 classes: LIP's count."""
import numpy as np
from torch.utils.data import Dataset


class SyntheticHumanParsingDataset(Dataset):

    def __init__(self, num_samples, height, width, num_classes=20, max_blobs=6, seed=0):
        self.num_samples, self.height, self.width = num_samples, height, width
        self.num_classes, self.max_blobs, self.seed = num_classes, max_blobs, seed
        self.palette = np.random.default_rng(seed).uniform(-2., 2., (num_classes, 3)).astype(np.float32)

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx):
        rng = np.random.default_rng((self.seed, idx))
        h, w = self.height, self.width
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        mask = np.zeros((h, w), dtype=np.float32)
        for _ in range(int(rng.integers(2, self.max_blobs + 1))):
            cy, cx = rng.uniform(0, h), rng.uniform(0, w)
            ry, rx = rng.uniform(h / 10 + 1, h / 3 + 1), rng.uniform(w / 10 + 1, w / 3 + 1)
            mask[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.] = float(rng.integers(1, self.num_classes))
        image = self.palette[mask.astype(np.int64)] + 0.5 * rng.standard_normal((h, w, 3), dtype=np.float32)
        return {'image': image.astype(np.float32), 'mask': mask, 'size': np.array([h, w], dtype=np.float32)}
