"""PFAN human parsing on the MI355X kernels -- drop-in for the reference module
SimpleAICV/human_parsing/models/pfan_human_parsing.py (PFANParsing :155, the 13 factories :330-400).

The reference module is its semantic-segmentation PFAN under another class name with num_classes = 20 (LIP's classes,
background included): PFANParsing here IS PFANSemanticSegmentation (semantic_segmentation/models/pfan_semantic_segmentation.py,
where the execution is described) with that default -- same constructor arguments, module tree, construction order (a seeded
construction draws the same initial weights), state_dict keys and `forward(x) -> [B, num_classes, H, W]`.
The DINOv3-ViT PFAN variant of the reference (dinov3_vit_pfan_human_parsing.py) is not built: the engine has no DINOv3 backbone."""
from ...semantic_segmentation.models.pfan_semantic_segmentation import PFANSemanticSegmentation

# backbone factory name and the four feature widths, per model prefix (the reference's 13)
PFAN_BACKBONES = {
    'resnet18': ('resnet18backbone', [64, 128, 256, 512]),
    'resnet34': ('resnet34backbone', [64, 128, 256, 512]),
    'resnet50': ('resnet50backbone', [256, 512, 1024, 2048]),
    'resnet101': ('resnet101backbone', [256, 512, 1024, 2048]),
    'resnet152': ('resnet152backbone', [256, 512, 1024, 2048]),
    'vanb0': ('vanb0backbone', [32, 64, 160, 256]),
    'vanb1': ('vanb1backbone', [64, 128, 320, 512]),
    'vanb2': ('vanb2backbone', [64, 128, 320, 512]),
    'vanb3': ('vanb3backbone', [64, 128, 320, 512]),
    'convformers18': ('convformers18backbone', [64, 128, 320, 512]),
    'convformers36': ('convformers36backbone', [64, 128, 320, 512]),
    'convformerm36': ('convformerm36backbone', [96, 192, 384, 576]),
    'convformerb36': ('convformerb36backbone', [128, 256, 512, 768]),
}


class PFANParsing(PFANSemanticSegmentation):
    """num_classes counts the background class."""

    def __init__(self, backbone_type, backbone_pretrained_path='', planes=[32, 64, 160, 256], cpfe_planes=32, num_classes=20,
                 use_gradient_checkpoint=False):
        super(PFANParsing, self).__init__(backbone_type, backbone_pretrained_path=backbone_pretrained_path, planes=planes,
                                          cpfe_planes=cpfe_planes, num_classes=num_classes,
                                          use_gradient_checkpoint=use_gradient_checkpoint)


def pfan_parsing_factories(suffix, num_classes):
    """-> {'<prefix>_pfan_<suffix>': factory(backbone_pretrained_path='', **kwargs)} for the 13 backbones; `num_classes` is the
    family's default and can be overridden per call, as in the reference"""

    def make(name, backbone_type, planes):
        def factory(backbone_pretrained_path='', **kwargs):
            kwargs.setdefault('num_classes', num_classes)
            return PFANParsing(backbone_type=backbone_type, backbone_pretrained_path=backbone_pretrained_path, planes=planes, **kwargs)

        factory.__name__ = factory.__qualname__ = name
        return factory

    return {f'{prefix}_pfan_{suffix}': make(f'{prefix}_pfan_{suffix}', bt, planes) for prefix, (bt, planes) in PFAN_BACKBONES.items()}


_FACTORIES = pfan_parsing_factories('human_parsing', 20)
globals().update(_FACTORIES)
__all__ = list(_FACTORIES)
