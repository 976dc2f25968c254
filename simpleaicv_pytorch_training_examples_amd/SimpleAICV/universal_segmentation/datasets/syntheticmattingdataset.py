"""Synthetic stand-in for the reference's HumanMattingDataset + transform block (universal_segmentation/datasets/
human_matting_dataset.py): a sample in the contract handed to the collaters of human_matting_common.py -- image, fg_map, bg_map
float32 HWC in [0, 255], mask the alpha matte float32 [H, W] in [0, 1], trimap uint8 [H, W] in {0, 128, 255}, size and origin_size
[h, w]."""
import numpy as np
from torch.utils.data import Dataset


class SyntheticUniversalMattingDataset(Dataset):
    """One soft-edged ellipse per sample: alpha falls from 1 inside to 0 outside over a band of `band` of the image side; the trimap
    is 255 where alpha is 1, 0 where it is 0 and 128 in between; image = alpha fg + (1 - alpha) bg of two noisy colours, so a model
    can learn the matte."""

    def __init__(self, num_samples, image_size=1024, band=0.08, seed=0, transform=None):
        self.num_samples, self.image_size, self.band, self.seed, self.transform = num_samples, image_size, band, seed, transform

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx):
        rng = np.random.default_rng((self.seed, idx))
        s = self.image_size
        cy, cx = rng.uniform(0.35 * s, 0.65 * s, 2)
        ry, rx = rng.uniform(0.15 * s, 0.3 * s, 2)
        ys, xs = np.mgrid[0:s, 0:s].astype(np.float32)
        dist = np.sqrt(((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2)
        alpha = np.clip((1. + self.band - dist) / (2 * self.band), 0., 1.).astype(np.float32)
        trimap = np.where(alpha >= 1., 255, np.where(alpha <= 0., 0, 128)).astype(np.uint8)
        fg = (rng.uniform(128, 255, 3)[None, None, :] + rng.uniform(-16, 0, (s, s, 3))).astype(np.float32)
        bg = (rng.uniform(0, 112, 3)[None, None, :] + rng.uniform(0, 16, (s, s, 3))).astype(np.float32)
        image = alpha[:, :, None] * fg + (1. - alpha[:, :, None]) * bg
        sample = {'image': image.astype(np.float32), 'mask': alpha, 'trimap': trimap, 'fg_map': fg, 'bg_map': bg,
                  'size': np.array([s, s], dtype=np.float32), 'origin_size': np.array([s, s], dtype=np.float32)}
        return self.transform(sample) if self.transform is not None else sample
