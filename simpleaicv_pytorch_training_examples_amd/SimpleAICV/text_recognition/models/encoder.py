"""BiLSTMEncoder of the reference (SimpleAICV/text_recognition/models/encoder.py): linear0, rnn1, linear1, rnn2, linear2 with the
reference's `state_dict` keys.  The three linear layers run on ops.linear; the two bidirectional LSTMs stay nn.LSTM (MIOpen)."""
import torch
import torch.nn as nn

from .... import ops

__all__ = [
    'BiLSTMEncoder',
]


def linear_frames(x, layer, out_f32=False):
    """x [B, T, C] -> [B, T, out] through ops.linear (a view when the out-features were padded: no copy of the 12 113-wide logits)"""
    b, t, c = x.shape
    x = x.reshape(b * t, c)
    if torch.is_autocast_enabled('cuda') and x.dtype != ops.compute_dtype():
        x = x.to(ops.compute_dtype())
    y = ops.linear(x, layer.weight, layer.bias, out_f32=out_f32)
    return y.view(b, t, y.shape[1]) if y.is_contiguous() else y.as_strided((b, t, y.shape[1]), (t * y.stride(0), y.stride(0), 1),
                                                                           y.storage_offset())


class BiLSTMEncoder(nn.Module):

    def __init__(self, inplanes, hidden_planes):
        super(BiLSTMEncoder, self).__init__()
        self.linear0 = nn.Linear(inplanes, hidden_planes)
        self.rnn1 = nn.LSTM(hidden_planes, hidden_planes, bidirectional=True, batch_first=True)
        self.linear1 = nn.Linear(hidden_planes * 2, hidden_planes)
        self.rnn2 = nn.LSTM(hidden_planes, hidden_planes, bidirectional=True, batch_first=True)
        self.linear2 = nn.Linear(hidden_planes * 2, hidden_planes)

    def forward(self, x):
        """x [B, T, C] -> [B, T, hidden_planes]"""
        x = linear_frames(x, self.linear0)
        self.rnn1.flatten_parameters()
        x, _ = self.rnn1(x)
        x = linear_frames(x, self.linear1)
        self.rnn2.flatten_parameters()
        x, _ = self.rnn2(x)
        return linear_frames(x, self.linear2)
