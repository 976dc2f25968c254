from .pfan_face_parsing import *
