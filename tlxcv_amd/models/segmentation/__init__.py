from .deeplab import deeplabv3, DeepLabV3, DeepLabV3Head, ASPPModule  # noqa: F401
from .resnet_vd import ResNet_vd  # noqa: F401

__all__ = ["deeplabv3", "DeepLabV3", "DeepLabV3Head", "ASPPModule", "ResNet_vd"]
