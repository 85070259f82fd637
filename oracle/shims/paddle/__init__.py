"""`paddle` names the reference's Paddle-converted model files touch on their eval-mode forward path
(swin_transformer.py:43-45,305; see ../README.md).  Development container only."""
import types

import torch

from oracle.tlx_cpu.pd import PdTensor, wrap

Tensor = PdTensor


def ones_like(x, dtype=None):
    return wrap(torch.ones_like(x))


def zeros_like(x, dtype=None):
    return wrap(torch.zeros_like(x))


def shape(x):
    return list(x.shape)


def rand(shape, dtype=None):
    return wrap(torch.rand(tuple(int(s) for s in shape)))


def to_tensor(data, dtype=None):
    return wrap(torch.as_tensor(data))


def matmul(a, b):          # gvt.py:69,120  tnt.py:107  levit.py:317
    return wrap(torch.matmul(a, b))


def transpose(x, perm):          # levit.py:317
    return wrap(x.permute(*perm))


def _unfold(x, kernel_sizes, strides=1, paddings=0, dilations=1):          # tnt.py:178
    return wrap(torch.nn.functional.unfold(x, kernel_sizes, dilation=dilations, padding=paddings, stride=strides))


nn = types.SimpleNamespace(functional=types.SimpleNamespace(unfold=_unfold))
