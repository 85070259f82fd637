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

DeepLabV3+ (deeplab.py:9-131, 247-309, 330-346; layer_libs.py:53-133) shares the backbone and the ASPP module, whose dilated
branches become SeparableConvBNReLU layers (depthwise 3x3 + BN, pointwise 1x1 + BN + ReLU: one engine.sepconv2d launch each, the
depthwise map kept on chip).  Its decoder concatenates without a pass too: the x2 bilinear resize of the ASPP output writes
columns 0-255 and conv_bn_relu1 (256 -> 48 on the stride-4 map) columns 256-303 of one [N, H/4, W/4, 304] buffer.
"""
import torch

from ... import engine as E
from ...tlx import nn
from .resnet_vd import ResNet_vd

__all__ = ["deeplabv3", "DeepLabV3", "DeepLabV3Head", "ASPPModule", "ConvBNReLU", "ConvBN", "SeparableConvBNReLU", "deeplabv3p",
           "DeepLabV3P", "DeepLabV3PHead", "Decoder"]


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


class ConvBN(nn.Module):
    """layer_libs.py:53-95: conv (bias unless bias_attr=False) -> BN."""

    def __init__(self, in_channels, out_channels, kernel_size, padding="same", stride=1, groups=1, dilation=1,
                 data_format="channels_first", **kwargs):
        super().__init__()
        b_init = False if kwargs.get("bias_attr", None) is False else "constant"
        self._conv = nn.GroupConv2d(padding=padding, dilation=dilation, in_channels=in_channels, out_channels=out_channels,
                                    kernel_size=kernel_size, n_group=groups, stride=stride, b_init=b_init, data_format=data_format)
        self.batch_norm = nn.BatchNorm2d(num_features=out_channels, data_format=data_format)

    def run_nhwc(self, v, **kw):
        return self._conv.run_nhwc(v, self.batch_norm, E.ACT_NONE, **kw)


class SeparableConvBNReLU(nn.Module):
    """layer_libs.py:98-133: depthwise ConvBN -> pointwise ConvBNReLU (the reference's attribute names, `piontwise_conv` included:
    they are the parameter tree)."""

    def __init__(self, in_channels, out_channels, kernel_size, padding="same", pointwise_bias=None, dilation=1,
                 data_format="channels_first", **kwargs):
        super().__init__()
        self.depthwise_conv = ConvBN(in_channels, out_channels=in_channels, kernel_size=kernel_size, padding=padding,
                                     groups=in_channels, dilation=dilation, data_format=data_format, **kwargs)
        self.piontwise_conv = ConvBNReLU(in_channels, out_channels, kernel_size=1, groups=1, bias_attr=pointwise_bias,
                                         data_format=data_format)

    def run_nhwc(self, v, out=None, out_ld=None):
        dw, pw = self.depthwise_conv._conv, self.piontwise_conv._conv
        if not (dw.kernel_size == (3, 3) and dw.stride == (1, 1) and dw.dilation[0] == dw.dilation[1]
                and dw.padding == dw.dilation and pw.padding == (0, 0) and pw.stride == (1, 1)):
            # not the 3x3 'same' form of DeepLabV3+: the two layers as they are
            kw = {} if out is None else {"out": out, "out_ld": out_ld}
            return self.piontwise_conv.run_nhwc(self.depthwise_conv.run_nhwc(v), **kw)
        dw._require_eval()
        pw._require_eval()
        w_dw = dw.packed()
        s1, t1 = dw.folded(self.depthwise_conv.batch_norm)
        pk = pw.packed()
        s2, t2 = pw.folded(self.piontwise_conv.batch_norm)
        return E.sepconv2d(v, w_dw, s1, t1, pk, s2, t2, dw.dilation[0], E.ACT_RELU, out=out, out_ld=out_ld)


class ASPPModule(nn.Module):
    """pyramid_pool.py:6-105 (use_sep_conv=True: DeepLabV3+, the dilated branches separable)."""

    def __init__(self, aspp_ratios, in_channels, out_channels, align_corners, use_sep_conv=False, image_pooling=False,
                 data_format="channels_first"):
        super().__init__()
        self.align_corners = align_corners
        self.data_format = data_format
        self.out_channels = out_channels
        self.aspp_blocks = nn.ModuleList()
        for ratio in aspp_ratios:
            conv_func = SeparableConvBNReLU if use_sep_conv and ratio > 1 else ConvBNReLU
            self.aspp_blocks.append(conv_func(in_channels=in_channels, out_channels=out_channels, kernel_size=1 if ratio == 1 else 3,
                                              dilation=ratio, padding=0 if ratio == 1 else ratio, data_format=data_format))
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


class Decoder(nn.Module):
    """deeplab.py:247-309."""

    def __init__(self, num_classes, in_channels, align_corners, data_format="channels_first", name=None):
        super().__init__(name=name)
        self.data_format = data_format
        self.conv_bn_relu1 = ConvBNReLU(in_channels=in_channels, out_channels=48, kernel_size=1, data_format=data_format)
        self.conv_bn_relu2 = SeparableConvBNReLU(in_channels=304, out_channels=256, kernel_size=3, padding=1, data_format=data_format)
        self.conv_bn_relu3 = SeparableConvBNReLU(in_channels=256, out_channels=256, kernel_size=3, padding=1, data_format=data_format)
        self.conv = nn.GroupConv2d(in_channels=256, out_channels=num_classes, kernel_size=1, data_format=data_format, padding=0)
        self.align_corners = align_corners

    def run_nhwc(self, x, low_level_feat):
        """x: the ASPP output (N, h, w, 256); low_level_feat: the stride-4 stage map (N, 2h, 2w, C) -> logits (N, 2h, 2w, classes).
        concat([resize(x), conv_bn_relu1(low)]) (deeplab.py:304) is one [N, 2h, 2w, 304] buffer both producers write into."""
        N, h, w, cx = x.shape
        H4, W4 = low_level_feat.shape[1], low_level_feat.shape[2]
        cat = torch.empty((N, H4, W4, cx + 48), dtype=x.dtype, device=x.device)
        E.resize_bilinear(x, (H4 / h, W4 / w), self.align_corners, out=cat[..., :cx])
        self.conv_bn_relu1.run_nhwc(low_level_feat, out=cat[..., cx:], out_ld=cx + 48)
        return self.conv.run_nhwc(self.conv_bn_relu3.run_nhwc(self.conv_bn_relu2.run_nhwc(cat)))


class DeepLabV3PHead(nn.Module):
    """deeplab.py:78-131."""

    def __init__(self, num_classes, backbone_indices, backbone_channels, aspp_ratios, aspp_out_channels, align_corners,
                 data_format="channels_first", name=None):
        super().__init__(name=name)
        self.aspp = ASPPModule(aspp_ratios, backbone_channels[1], aspp_out_channels, align_corners, use_sep_conv=True,
                               image_pooling=True, data_format=data_format)
        self.decoder = Decoder(num_classes, backbone_channels[0], align_corners, data_format=data_format)
        self.backbone_indices = backbone_indices

    def run_nhwc(self, feats):
        return self.decoder.run_nhwc(self.aspp.run_nhwc(feats[self.backbone_indices[1]]), feats[self.backbone_indices[0]])


class DeepLabV3P(nn.Module):
    """deeplab.py:9-75.  The factory keeps the reference's aspp_ratios=(1, 6, 12, 18) at output stride 8, although the docstring
    there suggests (1, 12, 24, 36)."""

    def __init__(self, num_classes, backbone, backbone_indices=(0, 3), aspp_ratios=(1, 6, 12, 18), aspp_out_channels=256,
                 align_corners=False, data_format="channels_first", name=None):
        super().__init__(name=name)
        if getattr(backbone, "output_stride", 8) != 8:
            raise NotImplementedError(f"DeepLabV3P: output_stride={backbone.output_stride} (only 8)")
        self.backbone = backbone
        backbone_channels = [backbone.feat_channels[i] for i in backbone_indices]
        self.head = DeepLabV3PHead(num_classes, backbone_indices, backbone_channels, aspp_ratios, aspp_out_channels, align_corners,
                                   data_format=data_format)
        self.align_corners = align_corners
        self.data_format = data_format

    @E.two_streams(1 << 30)       # as DeepLabV3: no half batches; the 2 GiB chunk step of two_streams() applies
    def forward(self, x):
        H, W = (x.shape[2], x.shape[3]) if self.data_format == "channels_first" else (x.shape[1], x.shape[2])
        if H % 8 or W % 8:
            raise NotImplementedError(f"DeepLabV3P: input {H}x{W}; H and W must be multiples of 8 (output stride 8, even extents "
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


def deeplabv3p(num_classes=19, backbone="ResNet50_vd", in_channels=3, output_stride=8, data_format="channels_first"):
    """deeplab.py:330-346."""
    if backbone != "ResNet50_vd":
        raise NotImplementedError(f"deeplabv3p: backbone {backbone!r} (only 'ResNet50_vd')")
    if output_stride != 8:
        raise NotImplementedError(f"deeplabv3p: output_stride={output_stride} (only 8)")
    bb = ResNet_vd(layers=50, in_channels=in_channels, output_stride=output_stride, data_format=data_format)
    return DeepLabV3P(num_classes=num_classes, backbone=bb, data_format=data_format)
