"""DeepLabV3 (ResNet50_vd backbone, output stride 8) on the MI355X engine.

Same factory, constructor arguments, attribute names and parameter tree as the reference
(tlxcv/models/segmentation/deeplab.py:134-189, 311-327; layers/pyramid_pool.py:6-105; layers/layer_libs.py:6-50), so one
weight dictionary fits both (the backbone's nested stage list registered as described in resnet_vd.py).  The forward is
NHWC from the stem to the classifier:
  * the ASPP branches write their 256-channel column slices of one [N, h, w, 1280] buffer through the output pitch — no
    concat pass; the image-pooling branch is global_avgpool -> 1x1 conv + BN + ReLU -> bilinear resize from 1 x 1 into slice 4;
  * projection 1x1 + BN + ReLU, dropout (the identity in eval), classifier 1x1 + bias;
  * the final bilinear resize to the input size writes the model's data_format directly (NCHW for channels_first).
Supported: output_stride 8 and inputs whose H and W are multiples of 8 (every stride-2 step sees an even extent and all resize
scales are exact); other output strides raise NotImplementedError.
"""
import torch

from ... import engine as E
from ...tlx import nn
from .resnet_vd import ResNet_vd

__all__ = ["deeplabv3", "DeepLabV3", "DeepLabV3Head", "ASPPModule", "ConvBNReLU"]


class ConvBNReLU(nn.Module):
    """layer_libs.py:6-50: conv (bias unless bias_attr=False) -> BN -> ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, padding="same", stride=1, groups=1, dilation=1,
                 data_format="channels_first", **kwargs):
        super().__init__()
        b_init = False if kwargs.get("bias_attr", None) is False else "constant"
        self._conv = nn.GroupConv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, padding=padding,
                                    stride=stride, n_group=groups, dilation=dilation, b_init=b_init, data_format=data_format)
        self.batch_norm = nn.BatchNorm2d(num_features=out_channels, data_format=data_format)

    def run_nhwc(self, v, **kw):
        return self._conv.run_nhwc(v, self.batch_norm, E.ACT_RELU, **kw)


class ASPPModule(nn.Module):
    """pyramid_pool.py:6-105 (use_sep_conv=False: DeepLabV3)."""

    def __init__(self, aspp_ratios, in_channels, out_channels, align_corners, use_sep_conv=False, image_pooling=False,
                 data_format="channels_first"):
        super().__init__()
        if use_sep_conv:
            raise NotImplementedError("ASPPModule: separable convs (DeepLabV3+) are not implemented")
        self.align_corners = align_corners
        self.data_format = data_format
        self.out_channels = out_channels
        self.aspp_blocks = nn.ModuleList()
        for ratio in aspp_ratios:
            self.aspp_blocks.append(ConvBNReLU(in_channels, out_channels, kernel_size=1 if ratio == 1 else 3, dilation=ratio,
                                               padding=0 if ratio == 1 else ratio, data_format=data_format))
        out_size = len(self.aspp_blocks)
        if image_pooling:
            self.global_avg_pool = nn.Sequential([
                nn.AdaptiveAvgPool2d(output_size=(1, 1), data_format=data_format),
                ConvBNReLU(in_channels, out_channels, kernel_size=1, bias_attr=False, data_format=data_format)])
            out_size += 1
        self.image_pooling = image_pooling
        self.conv_bn_relu = ConvBNReLU(out_channels * out_size, out_channels, kernel_size=1, data_format=data_format)
        self.dropout = nn.Dropout(p=0.1)

    def run_nhwc(self, v):
        N, h, w, _ = v.shape
        co = self.out_channels
        nb = len(self.aspp_blocks) + (1 if self.image_pooling else 0)
        cat = torch.empty((N, h, w, co * nb), dtype=v.dtype, device=v.device)
        for i, blk in enumerate(self.aspp_blocks):
            blk.run_nhwc(v, out=cat[..., i * co:(i + 1) * co], out_ld=co * nb)
        if self.image_pooling:
            g = E.global_avgpool(v).view(N, 1, 1, -1)
            g = self.global_avg_pool[1].run_nhwc(g)
            E.resize_bilinear(g, (h / 1, w / 1), self.align_corners, out=cat[..., (nb - 1) * co:])
        return self.conv_bn_relu.run_nhwc(cat)       # dropout: the identity in eval


class DeepLabV3Head(nn.Module):
    """deeplab.py:192-244."""

    def __init__(self, num_classes, backbone_indices, backbone_channels, aspp_ratios, aspp_out_channels, align_corners,
                 data_format="channels_first", name=None):
        super().__init__(name=name)
        self.aspp = ASPPModule(aspp_ratios, backbone_channels[0], aspp_out_channels, align_corners, use_sep_conv=False,
                               image_pooling=True, data_format=data_format)
        self.cls = nn.GroupConv2d(in_channels=aspp_out_channels, out_channels=num_classes, kernel_size=1, padding=0,
                                  data_format=data_format)
        self.backbone_indices = backbone_indices

    def run_nhwc(self, feats):
        return self.cls.run_nhwc(self.aspp.run_nhwc(feats[self.backbone_indices[0]]))


class DeepLabV3(nn.Module):
    """deeplab.py:134-189."""

    def __init__(self, num_classes, backbone, backbone_indices=(3,), aspp_ratios=(1, 6, 12, 18), aspp_out_channels=256,
                 align_corners=False, data_format="channels_first", name=None):
        super().__init__(name=name)
        if getattr(backbone, "output_stride", 8) != 8:
            # the size rule below (H, W multiples of 8) and the vd shortcut's 'SAME' pooling that pads nothing hold at output stride 8
            raise NotImplementedError(f"DeepLabV3: output_stride={backbone.output_stride} (only 8)")
        self.backbone = backbone
        backbone_channels = [backbone.feat_channels[i] for i in backbone_indices]
        self.head = DeepLabV3Head(num_classes, backbone_indices, backbone_channels, aspp_ratios, aspp_out_channels, align_corners,
                                  data_format=data_format)
        self.align_corners = align_corners
        self.data_format = data_format

    @E.two_streams(1 << 30)       # no half batches (not measured to pay); the 2 GiB chunk step of two_streams() applies
    def forward(self, x):
        H, W = (x.shape[2], x.shape[3]) if self.data_format == "channels_first" else (x.shape[1], x.shape[2])
        if H % 8 or W % 8:
            raise NotImplementedError(f"DeepLabV3: input {H}x{W}; H and W must be multiples of 8 (output stride 8, even extents "
                                      "at every stride-2 step)")
        v = nn.as_nhwc(x, self.data_format)
        logit = self.head.run_nhwc(self.backbone.features_nhwc(v))
        h, w = logit.shape[1], logit.shape[2]
        return E.resize_bilinear(logit, (H / h, W / w), self.align_corners,
                                 layout="nchw" if self.data_format == "channels_first" else "nhwc")


def deeplabv3(num_classes=19, backbone="ResNet50_vd", in_channels=3, output_stride=8, data_format="channels_first"):
    """deeplab.py:311-327."""
    if backbone != "ResNet50_vd":
        raise NotImplementedError(f"deeplabv3: backbone {backbone!r} (only 'ResNet50_vd')")
    if output_stride != 8:
        raise NotImplementedError(f"deeplabv3: output_stride={output_stride} (only 8)")
    bb = ResNet_vd(layers=50, in_channels=in_channels, output_stride=output_stride, data_format=data_format)
    return DeepLabV3(num_classes=num_classes, backbone=bb, data_format=data_format)
