"""Plain-torch restatement of DeepLabV3+ / ResNet50_vd (output stride 8) taking the parameter dictionary of the reference model
(tlxcv/models/segmentation/deeplab.py:9-131, 247-309; layers/layer_libs.py:53-133; layers/pyramid_pool.py), NCHW, any dtype and
device.  The backbone blocks, the BN and the conv helpers are deeplab_restated's; oracle/gen_golden.py checks this against
the reference file; the GPU tests use it for sizes without a golden.  Not a test module."""
import torch
import torch.nn.functional as F

import deeplab_restated as RS

seg_input = RS.seg_input


def backbone_feats(p, x, prefix="backbone."):
    """ResNet_vd.forward (backbones/resnet_vd.py:315-326): the four stage maps; the blocks as deeplab_restated.backbone runs them."""
    y = RS._conv_bn(p, prefix + "conv1_1", x, stride=2)
    y = RS._conv_bn(p, prefix + "conv1_2", y)
    y = RS._conv_bn(p, prefix + "conv1_3", y)
    y = F.max_pool2d(y, 3, 2, 1)
    feats = []
    for s, (n, dil) in enumerate(zip((3, 4, 6, 3), (1, 1, 2, 4))):
        for i in range(n):
            b = f"{prefix}stage_list_{s}_{i}."
            stride = 2 if i == 0 and s != 0 and dil == 1 else 1
            t = RS._conv_bn(p, b + "conv0", y)
            t = RS._conv_bn(p, b + "conv1", t, stride=stride, dilation=dil)
            t = RS._conv_bn(p, b + "conv2", t, relu=False)
            short = y if i > 0 else RS._conv_bn(p, b + "short", y, relu=False, vd=(s != 0 and stride == 2))
            y = F.relu(t + short)
        feats.append(y)
    return feats


def sep_conv(p, name, x, dilation=1, round_to=None):
    """SeparableConvBNReLU (layer_libs.py:98-133): depthwise 3x3 (padding = dilation, bias) + BN, then 1x1 (bias) + BN + ReLU.
    round_to: a dtype the depthwise map is rounded to before the 1x1 (the fp16 kernel's numerics), None for none."""
    w = p[f"{name}.depthwise_conv._conv.filters"]
    t = F.conv2d(x, w, p.get(f"{name}.depthwise_conv._conv.biases"), padding=dilation, dilation=dilation, groups=w.shape[0])
    t = RS._bn(p, f"{name}.depthwise_conv.batch_norm", t)
    if round_to is not None:
        t = t.to(round_to).to(x.dtype)
    return RS._conv_bn(p, f"{name}.piontwise_conv", t)


def deeplabv3p(p, x, align_corners=False):
    """x NCHW -> logits NCHW at the input size."""
    feats = backbone_feats(p, x)
    low, f = feats[0], feats[3]
    h = "head.aspp."
    outs = [RS._conv_bn(p, f"{h}aspp_blocks.0", f)]
    outs += [sep_conv(p, f"{h}aspp_blocks.{i}", f, dilation=r) for i, r in ((1, 6), (2, 12), (3, 18))]
    g = RS._conv_bn(p, f"{h}global_avg_pool.1", f.mean(dim=(2, 3), keepdim=True))
    outs.append(F.interpolate(g, scale_factor=(f.shape[2] / 1, f.shape[3] / 1), mode="bilinear", align_corners=align_corners))
    y = RS._conv_bn(p, f"{h}conv_bn_relu", torch.cat(outs, 1))
    d = "head.decoder."
    lo = RS._conv_bn(p, f"{d}conv_bn_relu1", low)
    y = F.interpolate(y, scale_factor=(lo.shape[2] / y.shape[2], lo.shape[3] / y.shape[3]), mode="bilinear",
                      align_corners=align_corners)
    y = torch.cat([y, lo], 1)
    y = sep_conv(p, f"{d}conv_bn_relu2", y)
    y = sep_conv(p, f"{d}conv_bn_relu3", y)
    y = F.conv2d(y, p[f"{d}conv.filters"], p[f"{d}conv.biases"])
    return F.interpolate(y, scale_factor=(x.shape[2] / y.shape[2], x.shape[3] / y.shape[3]), mode="bilinear",
                         align_corners=align_corners)
