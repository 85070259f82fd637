"""The `tlx_*` helpers as the reference's Paddle-converted files use them (../../../README.md lists who uses which).
tlx_Identity / tlx_Dropout are the identity in eval mode; the pools and the GELU are the stand-in's own layers, channels first."""
import torch

from oracle.tlx_cpu import nn


class tlx_Identity(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()

    def forward(self, x):
        return x


class tlx_Dropout(nn.Module):
    def __init__(self, p=0.5, *args, **kwargs):
        super().__init__()
        self.p = p

    def forward(self, x):
        assert not self.is_train or not self.p, "oracle stand-in is eval-only"
        return x


class tlx_GELU(nn.GELU):
    """Exact-erf GELU as a layer."""


class tlx_MaxPool2d(nn.MaxPool2d):
    """The padding takes no part in the max."""

    def __init__(self, kernel_size, stride, padding=0):
        super().__init__(kernel_size, stride, padding, data_format="channels_first")


class tlx_AvgPool2d(nn.AvgPool2d):
    """The zero padding counts in the divisor [TLX-recalled, as nn.AvgPool2d]."""

    def __init__(self, kernel_size, stride, padding=0):
        super().__init__(kernel_size, stride, padding, data_format="channels_first")


def tlx_linspace(start, stop, num):
    """`num` one-element rows: the callers iterate it and read `x.item()` (convnext.py:152, cswin_transformer.py:401),
    `x.numpy()[0]` (gvt.py:244) or keep `x` as the drop-path rate (van.py:186, pvt_v2.py:213)."""
    return list(torch.linspace(float(start), float(stop), int(num)).reshape(int(num), 1))


def tlx_get_tensor_shape(x):
    return tuple(x.shape)
