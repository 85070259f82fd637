from .deeplab import (deeplabv3, DeepLabV3, DeepLabV3Head, ASPPModule, deeplabv3p, DeepLabV3P, DeepLabV3PHead,  # noqa: F401
                      Decoder, SeparableConvBNReLU, ConvBN)
from .resnet_vd import ResNet_vd  # noqa: F401

__all__ = ["deeplabv3", "DeepLabV3", "DeepLabV3Head", "ASPPModule", "ResNet_vd", "deeplabv3p", "DeepLabV3P", "DeepLabV3PHead",
           "Decoder", "SeparableConvBNReLU", "ConvBN"]
