"""Synthetic stand-in for the reference's FaceParsingDataset + transform block in the benchmark configs: the samples of
SyntheticHumanParsingDataset (human_parsing/datasets/syntheticdataset.py) with 19 classes, CelebAMask-HQ's count."""
from ...human_parsing.datasets.syntheticdataset import SyntheticHumanParsingDataset


class SyntheticFaceParsingDataset(SyntheticHumanParsingDataset):

    def __init__(self, num_samples, height, width, num_classes=19, max_blobs=6, seed=0):
        super(SyntheticFaceParsingDataset, self).__init__(num_samples, height, width, num_classes=num_classes, max_blobs=max_blobs,
                                                          seed=seed)
