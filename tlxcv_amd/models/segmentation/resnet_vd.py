"""ResNet_vd backbone of the segmentation models on the MI355X engine.

Same constructor arguments, attribute names and parameter tree as the reference
(tlxcv/models/segmentation/backbones/resnet_vd.py:8-330), with one decision on top: the reference keeps its bottlenecks in
`self.stage_list`, a list of lists, which no module registry walks (its parameters and set_eval() would miss them).  Block i
of stage s is registered here as `stage_list_{s}_{i}` — the `{name}_{i}` rule of flat lists carried to nested ones
(DESIGN.md "DeepLabV3").  The forward is NHWC, one fused launch per conv + BN (+ ReLU) (+ residual);
at output stride 8 the 3x3 convs of stages 3 and 4 are dilated (2 and 4) and run on the gemm_pp convolution path.
"""
from ... import engine as E
from ...tlx import nn

__all__ = ["ResNet_vd", "ConvBNLayer", "BottleneckBlock"]


class ConvBNLayer(nn.Module):
    """resnet_vd.py:8-58: [avgpool 2/2 'SAME' (vd mode)] -> conv (no bias) -> BN -> act."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, dilation=1, groups=1, is_vd_mode=False, act=None,
                 data_format="channels_first"):
        super().__init__()
        if dilation != 1 and kernel_size != 3:
            raise RuntimeError("When the dilation isn't 1,the kernel_size should be 3.")
        self.is_vd_mode = is_vd_mode
        self._pool2d_avg = nn.AvgPool2d(kernel_size=2, stride=2, padding="SAME", data_format=data_format)
        self._conv = nn.GroupConv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride,
                                    padding=(kernel_size - 1) // 2 if dilation == 1 else dilation, dilation=dilation,
                                    data_format=data_format, b_init=False, n_group=groups)
        self.batch_norm = nn.BatchNorm2d(num_features=out_channels, data_format=data_format)
        self.act = act

    def run_nhwc(self, v, res=None, relu=None):
        """conv + BN (+ residual) (+ ReLU: the layer's own act, or `relu` when given) as one launch."""
        if self.is_vd_mode:
            v = self._pool2d_avg.run_nhwc(v)       # even extents: 'SAME' pads nothing (forward() checks H, W % 8)
        use_relu = (self.act == "relu") if relu is None else relu
        return self._conv.run_nhwc(v, self.batch_norm, E.ACT_RELU if use_relu else E.ACT_NONE, res=res)


class BottleneckBlock(nn.Module):
    """resnet_vd.py:61-130: 1x1 -> 3x3 (stride / dilation) -> 1x1 (x4), shortcut, add, ReLU — the add and the ReLU in conv2's
    epilogue."""

    def __init__(self, in_channels, out_channels, stride, shortcut=True, if_first=False, dilation=1, data_format="channels_first"):
        super().__init__()
        self.data_format = data_format
        self.conv0 = ConvBNLayer(in_channels, out_channels, 1, act="relu", data_format=data_format)
        self.dilation = dilation
        self.conv1 = ConvBNLayer(out_channels, out_channels, 3, stride=stride, act="relu", dilation=dilation, data_format=data_format)
        self.conv2 = ConvBNLayer(out_channels, out_channels * 4, 1, act=None, data_format=data_format)
        if not shortcut:
            self.short = ConvBNLayer(in_channels, out_channels * 4, 1, stride=1, is_vd_mode=False if if_first or stride == 1 else True,
                                     data_format=data_format)
        self.shortcut = shortcut

    def run_nhwc(self, v):
        t = self.conv1.run_nhwc(self.conv0.run_nhwc(v))
        short = v if self.shortcut else self.short.run_nhwc(v)
        return self.conv2.run_nhwc(t, res=short, relu=True)


class ResNet_vd(nn.Module):
    """resnet_vd.py:196-330, ResNet-50 and deeper (the bottleneck family DeepLabV3 uses)."""

    def __init__(self, layers=50, output_stride=8, multi_grid=(1, 1, 1), in_channels=3, data_format="channels_first"):
        super().__init__()
        self.data_format = data_format
        self.conv1_logit = None
        self.layers = layers
        self.output_stride = output_stride
        depths = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3], 152: [3, 8, 36, 3], 200: [3, 12, 48, 3]}
        if layers not in depths:
            raise NotImplementedError(f"ResNet_vd: layers={layers} (the engine runs the bottleneck depths {sorted(depths)})")
        depth = depths[layers]
        num_channels = [64, 256, 512, 1024]
        num_filters = [64, 128, 256, 512]
        self.feat_channels = [c * 4 for c in num_filters]
        dilation_dict = {2: 2, 3: 4} if output_stride == 8 else {3: 2} if output_stride == 16 else None
        self.conv1_1 = ConvBNLayer(in_channels, 32, 3, stride=2, act="relu", data_format=data_format)
        self.conv1_2 = ConvBNLayer(32, 32, 3, stride=1, act="relu", data_format=data_format)
        self.conv1_3 = ConvBNLayer(32, 64, 3, stride=1, act="relu", data_format=data_format)
        self.pool2d_max = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, data_format=data_format)
        self.stage_list = []
        for block in range(len(depth)):
            shortcut = False
            block_list = []
            for i in range(depth[block]):
                dilation_rate = dilation_dict[block] if dilation_dict and block in dilation_dict else 1
                if block == 3:
                    dilation_rate = dilation_rate * multi_grid[i]
                blk = BottleneckBlock(num_channels[block] if i == 0 else num_filters[block] * 4, num_filters[block],
                                      stride=2 if i == 0 and block != 0 and dilation_rate == 1 else 1, shortcut=shortcut,
                                      if_first=block == i == 0, dilation=dilation_rate, data_format=data_format)
                self.add_module(f"stage_list_{block}_{i}", blk)
                block_list.append(blk)
                shortcut = True
            self.stage_list.append(block_list)

    def features_nhwc(self, v):
        """NHWC input (channels padded to 16-byte chunks) -> the four stage outputs, NHWC."""
        v = self.conv1_3.run_nhwc(self.conv1_2.run_nhwc(self.conv1_1.run_nhwc(v)))
        v = self.pool2d_max.run_nhwc(v)
        feats = []
        for stage in self.stage_list:
            for blk in stage:
                v = blk.run_nhwc(v)
            feats.append(v)
        return feats

    def forward(self, x):
        v = nn.as_nhwc(x, self.data_format)
        return [nn.from_nhwc(f, self.data_format) for f in self.features_nhwc(v)]
