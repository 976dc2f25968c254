"""BiLSTMEncoder of the reference (SimpleAICV/text_recognition/models/encoder.py): linear0, rnn1, linear1, rnn2, linear2 with the
reference's `state_dict` keys.  The three linear layers run on ops.linear.  The two bidirectional LSTMs are nn.LSTM modules in
every case, so parameters, initialisation and checkpoints do not depend on the route: `rnn_route = 'library'` (the default) calls
them (MIOpen); `rnn_route = 'fused'` runs ops.lstm (csrc/lstm.hip) on their parameters -- no vendor GEMM, nothing read back,
bit-repeatable forward and backward.  CPU tensors go through the modules on either route."""
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
    rnn_route = 'library'

    def __init__(self, inplanes, hidden_planes, rnn_route=None):
        super(BiLSTMEncoder, self).__init__()
        if rnn_route is not None:
            self.rnn_route = rnn_route
        if self.rnn_route not in ('library', 'fused'):
            raise ValueError(f"BiLSTMEncoder: rnn_route {self.rnn_route!r}; 'library' or 'fused'")
        if self.rnn_route == 'fused' and not all(ops.lstm_supports(hidden_planes, hidden_planes, dt)
                                                 for dt in (torch.float32, torch.bfloat16)):
            raise ValueError(f'BiLSTMEncoder: the fused route does not run hidden_planes={hidden_planes} (ops.lstm_supports)')
        self.linear0 = nn.Linear(inplanes, hidden_planes)
        self.rnn1 = nn.LSTM(hidden_planes, hidden_planes, bidirectional=True, batch_first=True)
        self.linear1 = nn.Linear(hidden_planes * 2, hidden_planes)
        self.rnn2 = nn.LSTM(hidden_planes, hidden_planes, bidirectional=True, batch_first=True)
        self.linear2 = nn.Linear(hidden_planes * 2, hidden_planes)

    def _rnn(self, rnn, x):
        if self.rnn_route == 'fused' and x.is_cuda:
            return ops.lstm(x, dict(rnn.named_parameters()))
        rnn.flatten_parameters()
        return rnn(x)[0]

    def forward(self, x):
        """x [B, T, C] -> [B, T, hidden_planes]"""
        x = linear_frames(x, self.linear0)
        x = self._rnn(self.rnn1, x)
        x = linear_frames(x, self.linear1)
        x = self._rnn(self.rnn2, x)
        return linear_frames(x, self.linear2)
