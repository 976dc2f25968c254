"""Host side of the reference's text-recognition pipeline (SimpleAICV/text_recognition/common.py): Normalize (:525-540),
KeepRatioResizeTextRecognitionCollater (:543-575) and CTCTextLabelConverter (:578-650) with the reference's names, arguments and
results, plus the two string metrics its validation loop takes from other packages (edit distance, longest common subsequence),
written out here.  The reference's OpenCV augmentations (RandomScale ... Perspective) are not ported: the benchmark pipeline's
synthetic dataset delivers samples as they leave those transforms.  The collater's bilinear resize is torch's (half-pixel
centres, no antialiasing -- the sampling cv2.resize's INTER_LINEAR uses)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from ..classification.common import load_state_dict  # noqa: F401  (re-exported, as in the reference)


class Normalize:

    def __init__(self):
        pass

    def __call__(self, sample):
        sample['image'] = (sample['image'] / 255.).astype(np.float32)
        return sample


def _resize_hw(image, h, w):
    x = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).permute(2, 0, 1).unsqueeze(0)
    return F.interpolate(x, size=(h, w), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).numpy()


class KeepRatioResizeTextRecognitionCollater:
    """every image resized to height resize_h at its own aspect ratio, at the left of a zero canvas whose width is the batch's
    widest image rounded up to the next multiple of 32 (always at least one column of padding, as in the reference)"""

    def __init__(self, resize_h=32):
        self.resize_h = resize_h

    def __call__(self, data):
        images = [s['image'] for s in data]
        labels = [s['label'] for s in data]
        scales = [s['scale'] for s in data]
        sizes = [s['size'] for s in data]

        ratios = [image.shape[1] / float(image.shape[0]) for image in images]
        max_w = int(math.floor(max(ratios) * self.resize_h))
        max_w = int(((max_w // 32) + 1) * 32)

        input_images = np.zeros((len(images), self.resize_h, max_w, 3), dtype=np.float32)
        for i, image in enumerate(images):
            w = max(1, int(math.floor(self.resize_h * ratios[i])))
            if image.shape[0] != self.resize_h or image.shape[1] != w:
                image = _resize_hw(image, self.resize_h, w)
            input_images[i, 0:image.shape[0], 0:image.shape[1], :] = image
        # B H W 3 -> B 3 H W (the NCHW view of NHWC memory)
        input_images = torch.from_numpy(input_images).permute(0, 3, 1, 2).float()

        return {
            'image': input_images,
            'label': labels,
            'scale': scales,
            'size': sizes,
        }


class CTCTextLabelConverter:
    """text <-> class indices.  The characters take indices 0 .. len(chars) - 1, '[CTCblank]' the next one (= num_classes - 1);
    a character outside the table is the garbage class num_classes, which is why the model has num_classes + 1 outputs."""

    def __init__(self, chars_set_list, str_max_length=80, garbage_char='㍿'):
        self.ctc_chars_set = list(chars_set_list) + ['[CTCblank]']
        self.ctc_chars_dict = {char: i for i, char in enumerate(self.ctc_chars_set)}
        self.blank_index = self.ctc_chars_dict['[CTCblank]']
        self.str_max_length = str_max_length
        self.garbage_char = garbage_char
        self.num_classes = len(self.ctc_chars_set)

    def encode(self, text):
        """text: [batch] strings -> (indices int64 [batch, str_max_length] padded with the blank, lengths int32 [batch])"""
        length = [len(s) for s in text]
        batch_text = torch.LongTensor(len(text), self.str_max_length).fill_(self.blank_index)
        for i, t in enumerate(text):
            tmp = [self.ctc_chars_dict.get(char, self.num_classes) for char in t]
            batch_text[i][:len(tmp)] = torch.LongTensor(tmp)
        return batch_text, torch.IntTensor(length)

    def decode(self, text_index, length):
        """text_index [batch, T] per-frame classes, length [batch] -> strings: repeats collapsed, blanks dropped (index -1, what
        ops.ctc_greedy writes beyond a sample's frames, is dropped too)"""
        texts = []
        for index, l in enumerate(length):
            t = [int(v) for v in text_index[index, :int(l)]]
            char_list = []
            for i, v in enumerate(t):
                if v == self.num_classes:
                    char_list.append(self.garbage_char)
                if 0 <= v < self.num_classes - 1 and not (i > 0 and t[i - 1] == v):
                    char_list.append(self.ctc_chars_set[v])
            texts.append(''.join(char_list))
        return texts


def edit_distance(a, b):
    """Levenshtein distance of two sequences (insertions, deletions and substitutions cost 1)"""
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def lcs_length(a, b):
    """length of the longest common subsequence of two sequences"""
    prev = [0] * (len(b) + 1)
    for ca in a:
        cur = [0]
        for j, cb in enumerate(b, 1):
            cur.append(prev[j - 1] + 1 if ca == cb else max(prev[j], cur[j - 1]))
        prev = cur
    return prev[-1]
