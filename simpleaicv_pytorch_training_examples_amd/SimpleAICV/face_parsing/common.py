"""Batch collater of the face-parsing pipeline -- drop-in for the reference FaceParsingCollater (SimpleAICV/face_parsing/common.py),
the same contract as HumanParsingCollater (human_parsing/common.py): zero-padded image [B, 3, S, S], mask [B, S, S] float32 class
ids, size [B, 2] float32 (numpy)."""
from ..classification.common import load_state_dict  # noqa: F401  (re-exported, as in the reference)
from ..semantic_segmentation.common import SemanticSegmentationCollater


class FaceParsingCollater(SemanticSegmentationCollater):
    pass
