"""`tensorlayerx.ops` of the stand-in; the package's top level re-exports what the reference files also reach as `tensorlayerx.<name>`."""
import torch

from .nn import GELU as GeLU  # noqa: F401


def softmax(logits, axis=-1):
    return torch.softmax(logits, dim=axis)


def sigmoid(x):
    return torch.sigmoid(x)


def relu(x):
    return torch.relu(x)


def sqrt(x):
    return torch.sqrt(x)


def multiply(x, y):
    return x * y


def clip_by_value(t, clip_value_min, clip_value_max):
    return t.clamp(clip_value_min, clip_value_max)


def arange(start, limit=None, delta=1, dtype=None):
    return torch.arange(start, limit, delta, dtype=dtype) if limit is not None else torch.arange(start, dtype=dtype)


def stack(values, axis=0):
    return torch.stack(list(values), dim=axis)


def split(value, num_or_size_splits, axis=0):
    """An int means that many EQUAL sections (res2net.py:78), a list the section sizes (shufflenetv2.py:70, levit.py:205, mixnet.py:245)."""
    if isinstance(num_or_size_splits, int):
        return torch.chunk(value, num_or_size_splits, dim=axis)
    return torch.split(value, list(num_or_size_splits), dim=axis)


def squeeze(input, axis=None):
    """axis may be a list (squeezenet.py:158, ghostnet.py:63, googlenet.py:160 pass [2, 3])."""
    if axis is None:
        return input.squeeze()
    for a in sorted([axis] if isinstance(axis, int) else list(axis), reverse=True):
        input = input.squeeze(a)
    return input


def matmul(a, b, transpose_a=False, transpose_b=False):
    if transpose_a:
        a = a.transpose(-1, -2)
    if transpose_b:
        b = b.transpose(-1, -2)
    return torch.matmul(a, b)


def random_uniform(shape, minval=0, maxval=1, dtype=torch.float32, seed=None):
    return torch.rand(tuple(shape)) * (maxval - minval) + minval
