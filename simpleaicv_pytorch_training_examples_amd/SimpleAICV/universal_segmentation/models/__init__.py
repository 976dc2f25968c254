from .dinov3_universal_segmentation import *
# the matting factories are reached through their module (models.dinov3_universal_matting.__dict__[name]): the names of this package
# that start with dinov3_vit_ are the segmentation factories
from . import dinov3_universal_matting
from .dinov3_universal_matting import UniversalMatting
