"""CTCModel of the reference (SimpleAICV/text_recognition/models/ctc_model.py): backbone -> mean over the height -> BiLSTM encoder
-> predictor, images [B, 3, 32, W] -> logits [B, W / 8, num_classes]; the reference's constructor arguments and `state_dict` keys
(backbone.*, encoder.linear0 / rnn1 / linear1 / rnn2 / linear2, predictor.linear1 / linear2).  ConvFormer and VAN backbones are
not built."""
import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from . import backbones
from .encoder import BiLSTMEncoder
from .predictor import CTCPredictor

__all__ = [
    'CTCModel',
]


class CTCModel(nn.Module):

    def __init__(self, backbone_type, backbone_pretrained_path='', planes=256, num_classes=12114, use_gradient_checkpoint=False,
                 rnn_route='library'):
        super(CTCModel, self).__init__()
        self.use_gradient_checkpoint = use_gradient_checkpoint
        self.backbone = backbones.__dict__[backbone_type](**{
            'pretrained_path': backbone_pretrained_path,
            'use_gradient_checkpoint': use_gradient_checkpoint,
        })
        self.encoder = BiLSTMEncoder(inplanes=self.backbone.out_channels[-1], hidden_planes=planes, rnn_route=rnn_route)
        self.predictor = CTCPredictor(inplanes=planes, hidden_planes=planes, num_classes=num_classes)

    def forward(self, x):
        x = self.backbone(x)[-1]                         # [B, C, H', W'] (NHWC memory), H' = 2
        x = torch.mean(x, dim=2).permute(0, 2, 1)        # [B, W', C]
        if self.use_gradient_checkpoint:
            x = checkpoint(self.encoder, x, use_reentrant=False)
            return checkpoint(self.predictor, x, use_reentrant=False)
        return self.predictor(self.encoder(x))
