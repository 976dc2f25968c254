from .resnet import *
