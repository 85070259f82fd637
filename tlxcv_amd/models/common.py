"""What the model files share: one copy each of the small helpers that used to travel from one model file to the next.

The derived tensors of a conv / linear layer (packed filter, fp32 bias, folded BatchNorm) are not here: they are the layer's own
accessors (`GroupConv2d.packed / bias32 / folded / affine / dw_padded`, `Linear.packed / bias32` in tlx/nn), the only place their cache
keys are spelled.
"""
import torch

from .. import engine as E
from ..tlx import nn
from ..tlx.nn import as_nhwc, from_nhwc

__all__ = ['NHWCBlock', 'token_rows', 'pitched', 'act_code', 'make_divisible', 'drop_path', 'DropPath', 'Identity']

Identity = nn.Identity


class NHWCBlock(nn.Module):
    """forward() on a logical tensor in `self.data_format` ('channels_first' unless the class sets it) around run_nhwc(), which sees a
    dense NHWC map (a channel axis as_nhwc() has to pad is padded with zeros).  CROP: the map run_nhwc() returns is pitched wider than
    `self.out_channels`; forward() crops it."""
    data_format = 'channels_first'
    CROP = False

    def forward(self, x):
        self._require_eval()
        y = self.run_nhwc(as_nhwc(x, self.data_format))
        return from_nhwc(y, self.data_format, self.out_channels if self.CROP else None)


def token_rows(x, what):
    """(B, N, C) tokens in the engine's precision, dense."""
    E.need_gpu(x, "input")
    if x.dim() != 3:
        raise RuntimeError(f"{what}: (B, N, C) tokens are expected, got {tuple(x.shape)}")
    if x.dtype != E.precision():
        x = x.to(E.precision())
    return x if x.is_contiguous() else x.contiguous()


def pitched(like, H, W, channels, multiple):
    """A dense (N, H, W, roundup(channels, multiple)) buffer of `like`'s batch, dtype and device for a `channels`-wide map: zero filled
    where the pitch is wider than the map (whoever reads the whole pitch then reads zeros), uninitialised where it is not."""
    pitch = (channels + multiple - 1) // multiple * multiple
    make = torch.zeros if pitch != channels else torch.empty
    return make((like.shape[0], H, W, pitch), dtype=like.dtype, device=like.device)


def act_code(layer, what):
    """The engine's activation code of an activation layer or layer class: None and nn.Identity are ACT_NONE; `what` names the caller
    in the refusal of a layer the conv epilogue has no form of (no ACT, or a parameter such as LeakyReLU's slope)."""
    if layer is None or isinstance(layer, nn.Identity) or (isinstance(layer, type) and issubclass(layer, nn.Identity)):
        return E.ACT_NONE
    if not hasattr(layer, 'ACT') or getattr(layer, 'PARAM', 0.0):
        name = layer.__name__ if isinstance(layer, type) else type(layer).__name__
        raise NotImplementedError(f"{what}: activation {name} has no epilogue form")
    return layer.ACT


def make_divisible(v, divisor=8, min_value=None):
    """utils/common_func.py:1-16: the nearest multiple of `divisor`, at least `min_value` (default: `divisor`) and no less than 0.9 v."""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def drop_path(x, drop_prob=0.0, training=False):
    """Stochastic depth: the identity in eval mode, the only mode this engine runs."""
    if drop_prob == 0.0 or not training:
        return x
    raise RuntimeError("tlxcv_amd: drop_path in training mode — this engine runs eval-mode forward passes only")


class DropPath(nn.Module):
    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        return drop_path(x, self.drop_prob or 0.0, self.is_train)
