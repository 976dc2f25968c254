"""PFAN face parsing on the MI355X kernels -- drop-in for the reference module
SimpleAICV/face_parsing/models/pfan_face_parsing.py: the human-parsing PFAN (human_parsing/models/pfan_human_parsing.py) with
num_classes = 19 (CelebAMask-HQ's classes, background included) under the 13 `*_pfan_face_parsing` factory names.
The DINOv3-ViT PFAN variant of the reference (dinov3_vit_pfan_face_parsing.py) is not built."""
from ...human_parsing.models.pfan_human_parsing import PFANParsing, pfan_parsing_factories

_FACTORIES = pfan_parsing_factories('face_parsing', 19)
globals().update(_FACTORIES)
__all__ = list(_FACTORIES)
