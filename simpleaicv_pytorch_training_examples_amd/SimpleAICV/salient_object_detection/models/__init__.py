from .pfan_segmentation import *
