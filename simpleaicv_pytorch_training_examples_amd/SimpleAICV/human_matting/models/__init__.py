from .pfan_matting import *  # noqa: F401,F403
