"""Synthetic stand-in for the reference's HumanMattingDataset + transform block in the benchmark configs: a sample has the contract
the reference hands to HumanMattingCollater AFTER its transforms (human_matting/common.py:236-299): {'image', 'fg_map', 'bg_map':
float32 HWC, 'mask': float32 HW in [0, 1], 'trimap': uint8 HW with 0 / 128 / 255, 'size': [h, w]}.
The mask is one or two soft-edged ellipses; the trimap is derived from it as the reference derives it from the alpha matte (255
where the matte is opaque, 0 where it is empty, 128 in between, the band widened by a few pixels); the image is the composition
mask * fg + (1 - mask) * bg of a coloured foreground and a noise background, so a network can learn the mapping."""
import numpy as np
from torch.utils.data import Dataset


class SyntheticHumanMattingDataset(Dataset):

    def __init__(self, num_samples, height, width, max_objects=2, band=3, seed=0):
        self.num_samples, self.height, self.width = num_samples, height, width
        self.max_objects, self.band, self.seed = max_objects, band, seed
        self.colour = np.random.default_rng(seed).uniform(1., 2., 3).astype(np.float32)

    def __len__(self):
        return self.num_samples

    def _widen(self, region):
        """a boolean map grown by `band` pixels in the four axis directions (what the reference's dilate / erode pair does)"""
        out = region.copy()
        for s in range(1, self.band + 1):
            out[s:, :] |= region[:-s, :]
            out[:-s, :] |= region[s:, :]
            out[:, s:] |= region[:, :-s]
            out[:, :-s] |= region[:, s:]
        return out

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
        unknown = self._widen((mask > 0.) & (mask < 1.))
        trimap = np.where(unknown, 128, np.where(mask >= 1., 255, 0)).astype(np.uint8)
        fg = (self.colour + 0.25 * rng.standard_normal((h, w, 3), dtype=np.float32)).astype(np.float32)
        bg = (0.5 * rng.standard_normal((h, w, 3), dtype=np.float32)).astype(np.float32)
        image = mask[:, :, None] * fg + (1. - mask[:, :, None]) * bg
        return {'image': image.astype(np.float32), 'mask': mask, 'trimap': trimap, 'fg_map': fg, 'bg_map': bg,
                'size': np.array([h, w], dtype=np.float32)}
