"""ConvNeXt (ConvNeXt-T: depths 3/3/9/3, dims 96/192/384/768) forward graph on the MI355X engine.

Same factory / constructor arguments / attribute names / parameter tree as the reference
(tlxcv/models/classification/convnext.py:36-227; that file is a Paddle conversion that hard-imports `paddle`, so it is restated from
its text): 182 tensors, 28 589 128 values for the default 1000 classes, in the reference's order (a block's layer scale `gamma`
first, the channels-first norms own `weight` / `bias`).  Eval only; `drop_path_rate` is accepted and is the identity in eval.

Per block the reference does dwconv 7x7 -> permute -> LayerNorm -> Linear(C -> 4C) -> GELU -> Linear(4C -> C) -> * gamma -> permute
-> + input (:106-118).  Here the activations are NHWC throughout (no permutes) and, in fp16:
  * the depthwise conv runs on tlxmi_dwconv7_stats (the input tile staged in LDS once, the taps in registers), which also leaves
    the (sum, sum of squares) of every pixel's channels — the statistics of the LayerNorm that follows;
  * pwconv1 takes them and applies the LayerNorm in its epilogue, with GELU (engine.linear_ln: round 5's fold), so the block has no
    LayerNorm pass; where the fold's predicate says no (few rows) the LayerNorm launch stays;
  * pwconv2 adds bias, layer scale and the residual in its epilogue: y = (h W2) * gamma + gamma * b2 + input.  gamma stays an fp32
    per-channel scale — the reference initialises it to 1e-6 (:89), and 0.02 * 1e-6 is below the smallest fp16 subnormal, so it
    must not be multiplied into the fp16 filter.
The stem (conv 4x4 / 4 + channels-first LayerNorm, :141-143) is Swin's patch embedding (tlxmi_patch_embed4: the same arithmetic per
pixel); a downsample layer (:146-149) is a LayerNorm launch and the 2x2 / 2 conv; the tail is global_avgpool -> LayerNorm -> head.
fp32 (the parity mode) runs layer by layer on the generic kernels.
"""
import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc, from_nhwc
from ..common import DropPath, NHWCBlock, drop_path  # noqa: F401  (DropPath, drop_path: re-exported)

__all__ = ["ConvNeXt", "convnext", "Block", "ChannelsFirstLayerNorm", "DropPath", "drop_path"]

trunc_normal_ = nn.initializers.TruncatedNormal(stddev=0.02)
zeros_ = nn.initializers.Constant(value=0.0)
ones_ = nn.initializers.Constant(value=1.0)


class ChannelsFirstLayerNorm(nn.Module):
    """LayerNorm over the channel axis of a (B, C, H, W) tensor (convnext.py:52-74): per pixel, biased variance — nn.LayerNorm on
    the NHWC rows the engine keeps."""

    def __init__(self, normalized_shape, epsilon=1e-05):
        super().__init__()
        self.weight = nn.Parameter(data=ones_(shape=(normalized_shape,)))
        self.bias = nn.Parameter(data=zeros_(shape=(normalized_shape,)))
        self.epsilon = epsilon
        self.normalized_shape = [normalized_shape]

    def run_nhwc(self, v):
        return E.layernorm(v, self.weight.detach(), self.bias.detach(), self.epsilon)

    def forward(self, x):
        return from_nhwc(self.run_nhwc(as_nhwc(x, "channels_first")), "channels_first")


class Block(NHWCBlock):
    """convnext.py:77-118."""

    def __init__(self, dim, drop_path=0.0, layer_scale_init_value=1e-06):
        super().__init__()
        if layer_scale_init_value > 0:      # (first: the reference creates it after the layers, but a module's own parameters
            self.gamma = nn.Parameter(data=nn.initializers.Constant(value=layer_scale_init_value)(shape=(dim,)))   # precede its children's)
        else:
            self.gamma = None
        self.dwconv = nn.GroupConv2d(padding=3, in_channels=dim, out_channels=dim, kernel_size=7, n_group=dim,
                                     data_format='channels_first', W_init=trunc_normal_)
        self.norm = nn.LayerNorm(dim, epsilon=1e-06)
        self.pwconv1 = nn.Linear(in_features=dim, out_features=4 * dim, W_init=trunc_normal_)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(in_features=4 * dim, out_features=dim, W_init=trunc_normal_)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

    def run_nhwc(self, x):
        """x (B, H, W, C) NHWC in the engine's precision -> the block's output, same shape."""
        self._require_eval()
        dt = E.precision()
        B, H, W, C = x.shape
        dw, fc1 = self.dwconv, self.pwconv1
        w_rsc, b_dw = dw.packed(), dw.bias32()
        fused = E.dwconv7_supported(x)
        fold = fused and E.linear_ln_supported(B * H * W, C, fc1.out_features, dt, act=E.ACT_GELU)
        y, part = E.dwconv7_stats(x, w_rsc, b_dw, stats=fold, fused=fused)          # :108
        if part is not None:
            h = fc1.run_ln(y, self.norm, part, act=E.ACT_GELU)                      # :110-112, the LayerNorm inside pwconv1's epilogue
        else:
            h = fc1.run(self.norm(y), act=E.ACT_GELU)
        return self.scaled_fc2(h, x)

    def scaled_fc2(self, h, res=None):
        """gamma * (h W2 + b2) (+ res) as ONE epilogue (:113-117): gamma is the fp32 per-channel scale, gamma * b2 the shift."""
        fc2 = self.pwconv2
        pk2 = fc2.packed()
        if self.gamma is not None:
            def build():
                g = E._f32(self.gamma)
                b2 = E._f32(fc2.biases) if fc2.biases is not None else torch.zeros_like(g)
                return g.contiguous(), (g * b2).contiguous()
            scale, shift = self._cached("layer_scale", build, deps=(fc2,))
        else:
            scale, shift = None, fc2.bias32()
        return E.conv2d(h, pk2, scale=scale, shift=shift, res=res)


class ConvNeXt(nn.Module):
    """convnext.py:121-200."""

    def __init__(self, in_chans=3, class_num=1000, depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], drop_path_rate=0.0,
                 layer_scale_init_value=1e-06, head_init_scale=1.0):
        super().__init__()
        self.in_chans = in_chans
        self.downsample_layers = nn.ModuleList()
        stem = nn.Sequential([nn.GroupConv2d(stride=4, in_channels=in_chans, out_channels=dims[0], kernel_size=4, padding=0,
                                             data_format='channels_first', W_init=trunc_normal_),
                              ChannelsFirstLayerNorm(dims[0], epsilon=1e-06)])
        self.downsample_layers.append(stem)
        for i in range(3):
            self.downsample_layers.append(nn.Sequential([
                ChannelsFirstLayerNorm(dims[i], epsilon=1e-06),
                nn.GroupConv2d(stride=2, in_channels=dims[i], out_channels=dims[i + 1], kernel_size=2, padding=0,
                               data_format='channels_first', W_init=trunc_normal_)]))
        self.stages = nn.ModuleList()
        dp_rates = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths))]
        cur = 0
        for i in range(4):
            self.stages.append(nn.Sequential([Block(dim=dims[i], drop_path=dp_rates[cur + j], layer_scale_init_value=layer_scale_init_value)
                                              for j in range(depths[i])]))
            cur += depths[i]
        self.norm = nn.LayerNorm(dims[-1], epsilon=1e-06)
        self.head = nn.Linear(in_features=dims[-1], out_features=class_num, W_init=trunc_normal_)
        with torch.no_grad():                                                       # :164-169
            self.head.weights.mul_(head_init_scale)
            self.head.biases.mul_(head_init_scale)

    def _stem(self, x):
        """(B, 3, H, W) -> (B, H/4, W/4, dims[0]) NHWC: conv 4x4 / 4 + the channels-first LayerNorm (:141-143)."""
        conv, norm = self.downsample_layers[0][0], self.downsample_layers[0][1]
        D = conv.out_channels
        H4, W4 = x.shape[2] // 4 * 4, x.shape[3] // 4 * 4
        if H4 == 0 or W4 == 0:
            raise RuntimeError(f"ConvNeXt: a {x.shape[2]} x {x.shape[3]} image is smaller than the 4 x 4 stem")
        if (H4, W4) != (x.shape[2], x.shape[3]):       # the stride-4 conv without padding never reads the last H % 4 rows / W % 4 columns
            x = x[:, :, :H4, :W4].contiguous()
        if (E.option("patch_embed4") and E.precision() == torch.float16 and self.in_chans == 3 and D in (96, 128, 192, 256) and x.shape[1] == 3
                and x.shape[2] % 4 == 0 and x.shape[3] % 4 == 0 and x.dtype in (torch.float16, torch.float32)
                and not x.permute(0, 2, 3, 1).is_contiguous()):
            # one pass over the image, as Swin's patch embedding: conv + bias + LayerNorm over the D channels of a pixel
            w64 = conv._cached("pe4", lambda: E.patch_embed4_filter(conv.filters))
            y = E.patch_embed4(x, w64, conv.bias32(), norm.weight.detach(), norm.bias.detach(), norm.epsilon)
            return y.view(x.shape[0], x.shape[2] // 4, x.shape[3] // 4, D)
        if not x.permute(0, 2, 3, 1).is_contiguous():
            y = conv.run_stem(x, 4)                                                # 4x4 / 4 conv == 1x1 conv on 48 folded channels
        else:
            y = conv.run_nhwc(as_nhwc(x, 'channels_first'))
        return norm.run_nhwc(y)

    def forward_features(self, x):
        self._require_eval()
        E.need_gpu(x, "input")
        if x.dim() != 4:
            raise RuntimeError(f"ConvNeXt: a (B, C, H, W) image batch is expected, got {tuple(x.shape)}")
        y = self._stem(x)
        for i in range(4):                                                          # :192-194
            if i:
                norm, conv = self.downsample_layers[i][0], self.downsample_layers[i][1]
                y = conv.run_nhwc(norm.run_nhwc(y))
            for blk in self.stages[i]:
                y = blk.run_nhwc(y)
        return self.norm(E.global_avgpool(y))                                       # :195

    @E.two_streams(32, plan=None)
    def forward(self, x):
        return self.head.run(self.forward_features(x))


def _convnext(arch, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return ConvNeXt(depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], **kwargs)


def convnext(pretrained=False, **kwargs):
    """ConvNeXt-T (convnext.py:210-227)."""
    return _convnext('ConvNeXt_tiny', pretrained, **kwargs)
