from .sam_matting import *
