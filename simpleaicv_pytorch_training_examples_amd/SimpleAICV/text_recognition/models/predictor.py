"""CTCPredictor of the reference (SimpleAICV/text_recognition/models/predictor.py): two linear layers on ops.linear.  The second
has num_classes (12 113) out-features: ops.linear pads them to the 16-byte chunk and returns the view of the first num_classes, so
the logits' rows start 16-byte aligned and are never copied."""
import torch.nn as nn

from .encoder import linear_frames

__all__ = [
    'CTCPredictor',
]


class CTCPredictor(nn.Module):

    def __init__(self, inplanes, hidden_planes, num_classes):
        super(CTCPredictor, self).__init__()
        self.linear1 = nn.Linear(inplanes, hidden_planes)
        self.linear2 = nn.Linear(hidden_planes, num_classes)

    def forward(self, x):
        return linear_frames(linear_frames(x, self.linear1), self.linear2)
