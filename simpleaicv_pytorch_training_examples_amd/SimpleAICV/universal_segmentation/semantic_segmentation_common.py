"""Collaters of the universal-segmentation semantic task (reference SimpleAICV/universal_segmentation/semantic_segmentation_common.py:
SemanticSegmentationTestCollater :119, SemanticSegmentationTrainCollater :158) and the transforms the synthetic dataset needs
(RandomHorizontalFlip :16, Normalize :102; the OpenCV resizes are not ported: the synthetic samples are made at their final size).

A sample is {'image': float32 HWC, 'mask': a [H, W] label map with 0 = background, 'size', 'origin_size'}.  The train collater
turns a label map into one binary mask per class present (sorted ids, background removed, ids shifted by -1 so that the model's
last class is the no-object class); an all-background map raises, as the reference's np.stack of an empty list does."""
import numpy as np
import torch

from ..classification.common import load_state_dict  # noqa: F401  (re-exported, as in the reference)


class RandomHorizontalFlip:

    def __init__(self, prob=0.5):
        self.prob = prob

    def __call__(self, sample):
        if np.random.uniform(0, 1) < self.prob:
            sample['image'] = sample['image'][:, ::-1, :]
            sample['mask'] = sample['mask'][:, ::-1]
        return sample


class Normalize:

    def __call__(self, sample):
        sample['image'] = sample['image'] / 255.
        return sample


def _pad_images(images, resize):
    out = np.zeros((len(images), resize, resize, 3), dtype=np.float32)
    for i, image in enumerate(images):
        out[i, 0:image.shape[0], 0:image.shape[1], :] = image
    return torch.from_numpy(out).permute(0, 3, 1, 2).float()


class SemanticSegmentationTestCollater:

    def __init__(self, resize=512):
        self.resize = resize

    def __call__(self, data):
        masks = [s['mask'] for s in data]
        input_masks = np.zeros((len(masks), self.resize, self.resize), dtype=np.float32)      # 0 is the background class
        for i, per_mask in enumerate(masks):
            input_masks[i, 0:per_mask.shape[0], 0:per_mask.shape[1]] = per_mask
        return {
            'image': _pad_images([s['image'] for s in data], self.resize),
            'mask': torch.from_numpy(input_masks).float(),
            'size': np.array([s['size'] for s in data], dtype=np.float32),
            'origin_size': [s['origin_size'] for s in data],
        }


class SemanticSegmentationTrainCollater:

    def __init__(self, resize=512):
        self.resize = resize

    def __call__(self, data):
        input_masks, input_labels = [], []
        for s in data:
            per_mask = s['mask']
            class_ids = [v for v in np.unique(per_mask) if v != 0]
            class_masks = np.stack([per_mask == v for v in class_ids], dtype=np.float32)      # raises on an all-background map
            padded = np.zeros((len(class_masks), self.resize, self.resize), dtype=np.float32)
            padded[:, 0:class_masks.shape[1], 0:class_masks.shape[2]] = class_masks
            input_masks.append(torch.from_numpy(padded).float())
            # foreground ids start at 0 in the predictions; num_classes - 1 is the background the loss fills in
            input_labels.append(torch.from_numpy(np.array(class_ids).astype(np.float32)).long() - 1)
        return {
            'image': _pad_images([s['image'] for s in data], self.resize),
            'mask': input_masks,
            'label': input_labels,
            'size': np.array([s['size'] for s in data], dtype=np.float32),
        }
