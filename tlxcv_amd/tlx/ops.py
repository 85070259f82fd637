"""`tensorlayerx.ops` subset (vision_transformer.py:70,118; swin_transformer.py:143-146)."""
import torch

from .. import engine as _E
from .nn import GELU as GeLU  # noqa: F401  tlx.ops.GeLU is used as a layer class (vision_transformer.py:70)


def softmax(logits, axis=-1):
    return _E.softmax(logits, axis)


def sigmoid(x):
    _E.need_gpu(x)
    return _E.act_flat(x, _E.ACT_SIGMOID)


def relu(x):
    _E.need_gpu(x)
    return _E.act_flat(x, _E.ACT_RELU)


def arange(start, limit=None, delta=1, dtype=None):
    return torch.arange(start, limit, delta, dtype=dtype) if limit is not None else torch.arange(start, dtype=dtype)


def stack(values, axis=0):
    return torch.stack(list(values), dim=axis)


def convert_to_tensor(value, dtype=None):
    from . import convert_to_tensor as c
    return c(value, dtype)


class Resize:
    """tlx.Resize(scale, method, antialias, data_format) — deeplab.py:177-182, pyramid_pool.py:94-99.  [TLX-recalled: the torch
    backend calls F.interpolate(x, scale_factor=scale, mode=method, align_corners=antialias), transposing to NCHW and back for
    channels_last.]  Here: one bilinear HIP launch (tlxmi_resize_bilinear) on the NHWC view of x, writing the caller's layout
    directly; fp16 / fp32 in, the same dtype out.  Only method="bilinear"."""

    def __init__(self, scale, method="bilinear", antialias=False, data_format="channels_first"):
        if method != "bilinear":
            raise NotImplementedError(f"tlx.Resize: method {method!r} (only 'bilinear')")
        if data_format not in ("channels_first", "channels_last"):
            raise ValueError(f"tlx.Resize: data_format {data_format!r}")
        self.scale = scale
        self.method = method
        self.antialias = bool(antialias)
        self.data_format = data_format

    def __call__(self, x):
        _E.need_gpu(x, "input")
        if x.dim() != 4 or x.dtype not in (torch.float16, torch.float32):
            raise NotImplementedError("tlx.Resize: 4-D fp16 / fp32 tensors only")
        if self.data_format == "channels_first":
            v = x.permute(0, 2, 3, 1)
            if not v.is_contiguous():
                v = v.contiguous()
            return _E.resize_bilinear(v, self.scale, self.antialias, layout="nchw")
        return _E.resize_bilinear(x.contiguous(), self.scale, self.antialias)
