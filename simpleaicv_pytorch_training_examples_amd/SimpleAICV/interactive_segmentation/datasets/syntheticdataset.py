"""Synthetic stand-in for the reference's SAMSegmentationDataset + transform block in the benchmark config: a sample has the
contract handed to SAMBatchCollater after the transforms (interactive_segmentation/common.py:129-232): image float32 HWC,
a binary ellipse mask, its box, one positive prompt point inside it, a noisy prompt box and the mask as prompt mask."""
import numpy as np
from torch.utils.data import Dataset


class SyntheticSAMDataset(Dataset):

    def __init__(self, num_samples, image_size=1024, seed=0):
        self.num_samples, self.image_size, self.seed = num_samples, image_size, seed

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx):
        rng = np.random.default_rng((self.seed, idx))
        s = self.image_size
        image = rng.standard_normal((s, s, 3), dtype=np.float32)
        cy, cx = rng.uniform(0.3, 0.7, 2) * s
        ry, rx = rng.uniform(0.08, 0.25, 2) * s
        yy, xx = np.mgrid[0:s, 0:s]
        mask = ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0).astype(np.float32)
        box = np.array([cx - rx, cy - ry, cx + rx, cy + ry], dtype=np.float32)
        noise = rng.uniform(-0.1, 0.1, 4).astype(np.float32) * np.array([2 * rx, 2 * ry, 2 * rx, 2 * ry], dtype=np.float32)
        return {'image': image, 'box': box, 'mask': mask, 'size': np.array([s, s], dtype=np.float32),
                'prompt_point': np.array([[cx, cy, 1.0]], dtype=np.float32),
                'prompt_box': np.clip(box + noise, 0, s - 1).astype(np.float32), 'prompt_mask': mask}


class SyntheticSAMMattingDataset(Dataset):
    """Stand-in for the reference's SAMMattingDataset + transform block: a sample in the contract handed to SAMMattingBatchCollater
    (interactive_segmentation/common_matting.py): the SAM keys with `mask` a SOFT alpha in [0, 1] (an ellipse with a linear edge),
    `trimap` uint8 (0 outside, 255 where alpha is 1, 128 on the edge band), `fg_map` / `bg_map` float32 HWC and `image` their
    composition through alpha.  points_num positive prompt points lie inside the opaque core."""

    def __init__(self, image_size=1024, length=64, points_num=1, seed=0):
        self.image_size, self.length, self.points_num, self.seed = image_size, length, points_num, seed

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        rng = np.random.default_rng((self.seed, idx))
        s = self.image_size
        cy, cx = rng.uniform(0.3, 0.7, 2) * s
        ry, rx = rng.uniform(0.12, 0.25, 2) * s
        yy, xx = np.mgrid[0:s, 0:s]
        radius = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        alpha = np.clip((1.0 - radius) / 0.25, 0., 1.).astype(np.float32)          # 1 inside radius 0.75, 0 beyond 1
        trimap = np.full((s, s), 128, dtype=np.uint8)
        trimap[alpha <= 0.] = 0
        trimap[alpha >= 1.] = 255
        fg = rng.standard_normal((s, s, 3), dtype=np.float32)
        bg = rng.standard_normal((s, s, 3), dtype=np.float32)
        image = alpha[:, :, None] * fg + (1. - alpha[:, :, None]) * bg
        box = np.array([cx - rx, cy - ry, cx + rx, cy + ry], dtype=np.float32)
        noise = rng.uniform(-0.1, 0.1, 4).astype(np.float32) * np.array([2 * rx, 2 * ry, 2 * rx, 2 * ry], dtype=np.float32)
        offs = rng.uniform(-0.4, 0.4, (self.points_num, 2)) * np.array([rx, ry])
        points = np.concatenate([np.array([cx, cy]) + offs, np.ones((self.points_num, 1))], axis=1).astype(np.float32)
        return {'image': image, 'box': box, 'mask': alpha, 'size': np.array([s, s], dtype=np.float32), 'prompt_point': points,
                'prompt_box': np.clip(box + noise, 0, s - 1).astype(np.float32), 'prompt_mask': alpha.copy(), 'trimap': trimap,
                'fg_map': fg, 'bg_map': bg}
