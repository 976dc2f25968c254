"""Batch collater of the human-parsing pipeline -- drop-in for the reference HumanParsingCollater
(SimpleAICV/human_parsing/common.py:317-349), which is its semantic-segmentation collater under another name: images at the
top-left of a zero [B, S, S, 3] canvas handed over as its NCHW view, masks [B, S, S] float32 class ids padded with 0 (the
background class), sizes [B, 2] float32 (numpy) -- the un-padded (h, w) the evaluation crops to.  The reference's OpenCV
transforms (RandomCrop, RandomShrink, YoloStyleResize, Normalize, ...) are not part of the benchmark pipeline, whose synthetic
dataset delivers samples as they leave those transforms."""
from ..classification.common import load_state_dict  # noqa: F401  (re-exported, as in the reference)
from ..semantic_segmentation.common import SemanticSegmentationCollater


class HumanParsingCollater(SemanticSegmentationCollater):
    pass
