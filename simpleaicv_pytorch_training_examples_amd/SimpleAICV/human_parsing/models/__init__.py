from .pfan_human_parsing import *
