from .ctc_model import *
