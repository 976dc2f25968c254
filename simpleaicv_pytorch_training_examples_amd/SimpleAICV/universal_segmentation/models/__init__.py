from .dinov3_universal_segmentation import *
