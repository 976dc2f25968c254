"""Synthetic stand-in for the reference's text-recognition datasets in benchmark configs: a sample has the contract the reference
hands to KeepRatioResizeTextRecognitionCollater AFTER its transforms (text_recognition/common.py:543-575): {'image': float32 HWC in
[0, 1], 'label': the text, 'scale': 1.0, 'size': [h, w]}.  The label is a random string of 1 to max_length characters of the given
table; the image shows it: the width is cut into one cell per character and each cell carries its character's colour pattern
(three stripes whose intensities are digits of the character's index) under noise, so a network can learn to read it.  Fixed
width by default (the benchmark's 32 x 512); `variable_width=True` draws a width per sample from width // 2 to width."""
import numpy as np
from torch.utils.data import Dataset


class SyntheticTextRecognitionDataset(Dataset):

    def __init__(self, num_samples, chars, height=32, width=512, max_length=24, variable_width=False, seed=0):
        self.num_samples, self.chars = num_samples, list(chars)
        self.height, self.width, self.max_length = height, width, max_length
        self.variable_width, self.seed = variable_width, seed

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx):
        rng = np.random.default_rng((self.seed, idx))
        n = int(rng.integers(1, self.max_length + 1))
        ids = rng.integers(0, len(self.chars), n)
        w = int(rng.integers(self.width // 2, self.width + 1)) if self.variable_width else self.width
        h = self.height
        image = np.zeros((h, w, 3), dtype=np.float32)
        edges = np.linspace(0, w, n + 1).astype(np.int64)
        rows = np.linspace(0, h, 4).astype(np.int64)
        for k, c in enumerate(ids):
            digits = [(int(c) // 23 ** j) % 23 for j in range(3)]                # three base-23 digits cover 12 167 characters
            for j in range(3):
                image[rows[j]:rows[j + 1], edges[k]:edges[k + 1], :] = (digits[j] + 1) / 24.0
                image[rows[j]:rows[j + 1], edges[k]:edges[k + 1], j] = 1.0      # which stripe: one channel saturated
        image = np.clip(image + 0.02 * rng.standard_normal(image.shape, dtype=np.float32), 0.0, 1.0)
        return {'image': image, 'label': ''.join(self.chars[int(c)] for c in ids), 'scale': np.float32(1.0),
                'size': np.array([h, w], dtype=np.float32)}
