from .resnet import (ResNet, resnet18, resnet34, resnet50, resnet101, resnet152, wide_resnet50_2,  # noqa: F401
                     wide_resnet101_2)
from .vision_transformer import (VisionTransformer, vit_small_patch16_224, vit_base_patch16_224,  # noqa: F401
                                 vit_base_patch16_384, vit_base_patch32_384, vit_large_patch16_224,
                                 vit_large_patch16_384, vit_large_patch32_384)
from .swin_transformer import (SwinTransformer, swintransformer_tiny_patch4_window7_224,  # noqa: F401
                               swintransformer_small_patch4_window7_224, swintransformer_base_patch4_window7_224,
                               swintransformer_large_patch4_window7_224, swintransformer_base_patch4_window12_384,
                               swintransformer_large_patch4_window12_384)
from .mobilenetv1 import MobileNetV1  # noqa: F401
from .mobilenetv2 import (MobileNetV2, mobilenet_v2, MobileNetV3Small, MobileNetV3Large, mobilenet_v3_small,  # noqa: F401
                          mobilenet_v3_large)
from .vgg import VGG, vgg11, vgg13, vgg16, vgg19  # noqa: F401
from .alexnet import AlexNet, alexnet  # noqa: F401
from .resnext import (ResNeXt, resnext50_32x4d, resnext50_64x4d, resnext101_32x4d, resnext101_64x4d,  # noqa: F401
                      resnext152_32x4d, resnext152_64x4d)
from .efficientnet import efficientnet, EfficientNet  # noqa: F401
from .resnest import resnest50_fast_1s1x64d, resnest50, resnest101, ResNeSt  # noqa: F401
from .convnext import ConvNeXt, convnext, Block, ChannelsFirstLayerNorm, DropPath  # noqa: F401
from .densenet import (DenseNet, densenet121, densenet161, densenet169, densenet201, densenet264, BNACConvLayer, DenseLayer,  # noqa: F401
                       DenseBlock, TransitionLayer, ConvBNLayer)
# (the PVTv2 file's Mlp / Attention / Block / DWConv stay in their module: ConvNeXt's Block and DropPath own those names here)
from .pvt_v2 import PyramidVisionTransformerV2, pvt_v2, OverlapPatchEmbed  # noqa: F401
# (the VAN file's Mlp / LKA / Attention / Block / OverlapPatchEmbed / DWConv stay in their module, like PVTv2's)
from .van import VAN, VAN_B0, van  # noqa: F401
# (the CSWin file's Mlp stays in its module)
from .cswin_transformer import (CSwinTransformer, CSwintransformer_thiny, PatchEmbedding, LePEAttention, CSwinBlock, MergeBlock,  # noqa: F401
                                CSwinStage)
# (the LeViT file's Attention / Residual / Subsample stay in their module: PVTv2's and VAN's own those names in theirs)
from .levit import (LeViT, levit_128s, levit_128, levit_192, levit_256, levit_384, AttentionSubsample, Conv2d_BN, Linear_BN,  # noqa: F401
                    BN_Linear, b16)
# (the TNT file's Block / Attention / Mlp stay in their module: ConvNeXt's Block owns that name here, and the other two follow PVTv2's rule)
from .tnt import TNT, PixelEmbed, tnt_small  # noqa: F401
# (the Twins file's Attention / Block / PatchEmbed stay in their module: PVTv2's, ConvNeXt's and ViT's own those names in theirs)
from .shufflenetv2 import (ShuffleNetV2, InvertedResidual, InvertedResidualDS, create_activation_layer, channel_shuffle,  # noqa: F401
                           shufflenet_v2_x0_25, shufflenet_v2_x0_33, shufflenet_v2_x0_5, shufflenet_v2_x1_0, shufflenet_v2_x1_5,
                           shufflenet_v2_x2_0, shufflenet_v2_swish)
from .ghostnet import (GhostNet, GhostBottleneck, GhostModule, SEBlock, ghostnet_x0_5, ghostnet_x1_0, ghostnet_x1_3)  # noqa: F401
from .gvt import (GroupAttention, SBlock, GroupBlock, PyramidVisionTransformer, PosCNN, CPVTV2, PCPVT, ALTGVT, pcpvt_small,  # noqa: F401
                  pcpvt_base, pcpvt_large, alt_gvt_small, alt_gvt_base, alt_gvt_large)
# (the MixNet file's ConvBlock / SEBlock / get_activation_layer stay in their module: GhostNet's SEBlock owns that name here)
from .mixnet import (MixNet, MixUnit, MixInitBlock, MixConv, MixConvBlock, mixconv1x1_block, round_channels, mixnet_s, mixnet_m,  # noqa: F401
                     mixnet_l)
# (the Res2Net file's ConvBNLayer / BottleneckBlock stay in their module: DenseNet's ConvBNLayer owns that name here)
from .res2net import Res2Net, res2net  # noqa: F401
from .googlenet import GoogLeNet, ConvLayer, Inception, googlenet  # noqa: F401
from .squeezenet import SqueezeNet, MakeFire, MakeFireConv, squeezenet1_0, squeezenet1_1  # noqa: F401
# (the DPN file's ConvBNLayer / BNACConvLayer stay in their module: DenseNet's own those names here)
from .dpn import DPN, DualPathFactory, dpn68, dpn107  # noqa: F401
# (the HarDNet file's ConvLayer stays in its module: GoogLeNet's owns that name here)
from .hardnet import HarDNet, HarDBlock, DWConvLayer, CombConvLayer, hardnet39, hardnet85  # noqa: F401
from .rexnet import ReXNetV1, LinearBottleneck, SE, rexnet_1_0, rexnet_1_3, rexnet_1_5, rexnet_2_0, rexnet_3_0  # noqa: F401
