"""Losses of the reference's face-parsing family (SimpleAICV/face_parsing/losses.py): the same four classes as human parsing's
(CELoss, MultiClassBCELoss, IoULoss, DiceLoss), one implementation -- see human_parsing/losses.py."""
from ..human_parsing.losses import CELoss, MultiClassBCELoss, IoULoss, DiceLoss

__all__ = [
    'CELoss',
    'MultiClassBCELoss',
    'IoULoss',
    'DiceLoss',
]
