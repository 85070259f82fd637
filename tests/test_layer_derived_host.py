"""CPU-side tests of the layers' derived-tensor accessors and of tlxcv_amd/models/common.py.

The cache keys of a conv / linear layer's own derived tensors ("pk", "dw", "gpk", "bias", ("bn", id), ("dw_padded", width)) are spelled
in tlxcv_amd/tlx/nn only: a model file or tool that calls `_cached` with one of them has copied the convention back, and the scan below
fails.  make_divisible is checked against the GhostNet widths worked out by hand in test_ghostnet_host.py, act_code on every activation
layer of nn."""
import ast
import glob
import importlib
import os

import pytest

from conftest import REPO
from test_ghostnet_host import SCALE, WIDTHS

LAYER_KEYS = ("pk", "dw", "gpk", "bias")
LAYER_TUPLE_KEYS = ("bn", "dw_padded")


def _layer_key_calls(path):
    """[(line, key)] of the `x._cached(<a layer's key>, ...)` calls in a source file."""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    found = []
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "_cached"):
            continue
        key = node.args[0] if node.args else next((k.value for k in node.keywords if k.arg == "key"), None)
        if isinstance(key, ast.Constant) and key.value in LAYER_KEYS:
            found.append((node.lineno, repr(key.value)))
        elif isinstance(key, ast.Tuple) and key.elts and isinstance(key.elts[0], ast.Constant) and key.elts[0].value in LAYER_TUPLE_KEYS:
            found.append((node.lineno, f"({key.elts[0].value!r}, ...)"))
    return found


def test_scan_finds_what_it_looks_for(tmp_path):
    src = tmp_path / "m.py"
    src.write_text('a = c._cached("pk", f)\nb = c._cached(("bn", id(bn)), f, deps=(bn,))\nd = c._cached(("dw_padded", 8), f)\n'
                   'e = c._cached(key="bias", build=f)\nok = c._cached(("pk", part), f)\nok2 = c._cached("se", f)\n')
    assert [line for line, _ in _layer_key_calls(str(src))] == [1, 2, 3, 4]


def test_no_layer_key_is_spelled_outside_the_layers():
    files = sorted(glob.glob(os.path.join(REPO, "tlxcv_amd", "models", "**", "*.py"), recursive=True)
                   + glob.glob(os.path.join(REPO, "tools", "*.py")))
    assert len(files) > 40
    bad = [f"{os.path.relpath(p, REPO)}:{line}: _cached({key}" for p in files for line, key in _layer_key_calls(p)]
    assert not bad, "use the layer's accessor (packed / bias32 / folded / affine / dw_padded):\n" + "\n".join(bad)


@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_make_divisible_gives_the_hand_worked_ghostnet_widths(name):
    from ghostnet_restated import CFGS
    from tlxcv_amd.models import GhostNet
    from tlxcv_amd.models.common import make_divisible
    scale = SCALE[name]
    stem, blocks, last = WIDTHS[name]
    assert make_divisible(16 * scale, 4) == stem
    for (cin, hid, out), (_, exp, c, _, _) in zip(blocks, CFGS):
        assert (make_divisible(exp * scale, 4), make_divisible(c * scale, 4)) == (hid, out)
    assert make_divisible(CFGS[-1][1] * scale, 4) == last
    assert GhostNet._make_divisible(None, CFGS[3][1] * scale, 4) == blocks[3][1]         # the reference's method name: a delegate
    # the default divisor (8), a floor, and the 0.9 v rule: 18 -> 16 would lose more than 10 %, so 24
    assert make_divisible(18) == 24 and make_divisible(19) == 24 and make_divisible(3) == 8 and make_divisible(3, 8, 16) == 16
    assert make_divisible(100, 8) == 104 and make_divisible(99.9, 8) == 96


def test_act_code_on_every_activation_layer():
    from tlxcv_amd import engine as E
    from tlxcv_amd.models.common import act_code
    from tlxcv_amd.tlx import nn
    codes = {nn.ReLU: E.ACT_RELU, nn.ReLU6: E.ACT_RELU6, nn.Hardswish: E.ACT_HARDSWISH, nn.HardSigmoid: E.ACT_HARDSIGMOID,
             nn.Sigmoid: E.ACT_SIGMOID, nn.Swish: E.ACT_SILU, nn.GELU: E.ACT_GELU}
    acts = [c for c in vars(nn).values() if isinstance(c, type) and issubclass(c, nn._Act) and c is not nn._Act]
    assert set(acts) == set(codes) | {nn.LeakyReLU}                   # a new activation layer gets its line here
    for cls, code in codes.items():
        assert act_code(cls, "t") == code and act_code(cls(), "t") == code
    assert act_code(None, "t") == E.ACT_NONE and act_code(nn.Identity, "t") == E.ACT_NONE and act_code(nn.Identity(), "t") == E.ACT_NONE
    # a slope is a parameter the callers' epilogues are not given: refused, the caller named
    with pytest.raises(NotImplementedError, match="Stem: activation LeakyReLU"):
        act_code(nn.LeakyReLU(0.1), "Stem")
    assert act_code(nn.LeakyReLU(0.0), "t") == E.ACT_LEAKY and act_code(nn.LeakyReLU, "t") == E.ACT_LEAKY      # no non-zero PARAM
    for layer in (nn.Softmax(), nn.Dropout(0.1), nn.Flatten, nn.Linear(in_features=4, out_features=4)):
        with pytest.raises(NotImplementedError, match="Head: activation"):
            act_code(layer, "Head")


def test_old_names_stay_importable():
    from tlxcv_amd.models import common
    convnext, swin_transformer, vision_transformer = (            # (a package attribute may be the factory of the same name)
        importlib.import_module("tlxcv_amd.models.classification." + m) for m in ("convnext", "swin_transformer", "vision_transformer"))
    from tlxcv_amd.tlx import nn
    assert vision_transformer.Identity is nn.Identity and common.Identity is nn.Identity
    for mod in (convnext, swin_transformer):
        assert mod.DropPath is common.DropPath and mod.drop_path is common.drop_path
    assert vision_transformer.DropPath is common.DropPath
    x = object()
    assert common.drop_path(x, 0.3, False) is x and common.drop_path(x, 0.0, True) is x
    with pytest.raises(RuntimeError, match="training mode"):
        common.drop_path(x, 0.3, True)
