from .pfan_semantic_segmentation import *
