"""Seeded, numpy-only weight and input recipes.

There is no network for checkpoints, so benches and parity tests fill models from these explicit
recipes: every value comes from `numpy.random.default_rng(seed)` (never torch's RNG), keyed by the
parameter's dotted attribute path, so the same dictionary loads into the engine's model, into the
CPU oracle, and — in the development container — into the reference's own model file.

The recipes are chosen so that activations keep O(1) magnitude through deep residual stacks (so the
fp16 throughput mode never saturates) while every BatchNorm statistic, bias and affine parameter
is non-trivial (so a parity test would catch a dropped or mis-ordered term).
"""
import re

import numpy as np

# Twins (gvt.py): blocks.<stage>.<index>.attn.{q, kv, qkv, proj} — the only tree whose blocks carry two indices
_TWINS_ATTN = re.compile(r"^blocks\.\d+\.\d+\.attn\.(q|kv|qkv|proj)$")
# GhostNet (ghostnet.py:109-126): the convs of a bottleneck that no ReLU follows
_GHOST_LINEAR = re.compile(r"^_ghostbottleneck_\d+\.(ghost_module_2\.(primary_conv|cheap_operation)|depthwise_conv|shortcut_depthwise|shortcut_conv)\._conv$")
# MixNet (mixnet.py:410-417, :449): a unit's projection conv2 — no activation follows it and it feeds the residual add
_MIXNET_PROJ = re.compile(r"^features\.(init_block\.conv2|stage\d+\.unit\d+)\.conv2\.")
# Res2Net (res2net.py:60-69): the 3x3 convs of the hierarchical chain, registered as bb_<b>_<i>.res<k><x>_branch2b_<s> — names no other
# tree has (ResNeXt's bb_<b>_<i> blocks keep conv0 / conv1 / conv2) — and the block's expand BatchNorm, which feeds the residual add
_RES2NET_CHAIN = re.compile(r"^bb_\d+_\d+\.res\d+\w*_branch2b_\d+\.")
_RES2NET_LAST_BN = re.compile(r"^bb_\d+_\d+\.conv2\.batch_norm$")
# SqueezeNet (squeezenet.py:37-46): a Fire module's expand 1x1, registered as _conv<k>._conv_path1 — a name no other tree has
_SQUEEZENET_FIRE = re.compile(r"^_conv\d+\._conv_path1\._conv\.")
# DPN (dpn.py:103-105, :121-126): a DualPathFactory's last conv, registered as dpn<k>.c1x1_c_func — a name no other tree has; its first
# bw output channels are added to the residual path, which nothing normalises
_DPN_C = re.compile(r"^dpn\d+\.c1x1_c_func\._conv\.")
DPN_C_GAIN = 0.6


def image_batch(n, seed=0, hw=224, c=3):
    """Synthetic ImageNet-shaped batch, NCHW fp32, roughly the range left by the demo's Normalize
    (demo/image_classification/predict.py:25): unit gaussian noise plus, per image and channel, a
    smooth plane wave of random frequency / phase / amplitude and a random DC offset, so different
    images drive a random-weight network to visibly different logits."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c, hw, hw), dtype=np.float32)
    yy, xx = np.meshgrid(np.arange(hw, dtype=np.float32), np.arange(hw, dtype=np.float32), indexing="ij")
    fy = rng.uniform(-0.2, 0.2, (n, c, 1, 1)).astype(np.float32)
    fx = rng.uniform(-0.2, 0.2, (n, c, 1, 1)).astype(np.float32)
    ph = rng.uniform(0, 2 * np.pi, (n, c, 1, 1)).astype(np.float32)
    amp = rng.uniform(0.5, 2.0, (n, c, 1, 1)).astype(np.float32)
    dc = rng.uniform(-1.0, 1.0, (n, c, 1, 1)).astype(np.float32)
    x += amp * np.sin(fy * yy + fx * xx + ph) + dc
    return np.ascontiguousarray(x, dtype=np.float32)


def _is_last_bn_of_block(name):
    # ResNet: bn3 of a bottleneck / bn2 of a basic block / the downsample BN feed the residual add;
    # DarkNet: the BatchNorm of BasicBlock.conv2 (darknet.py:142-153) does.
    # MobileNetV2/V3: the BatchNorm of the linear projection (mobilenetv2.py:30-33, mobilenetv3.py:107-110).
    # ResNeSt: conv3's BatchNorm and the shortcut BatchNorm of a bottleneck (resnest.py:258-309).
    if "_bottleneck_" in name and name.rsplit("_bottleneck_", 1)[1].split(".", 1)[1:] in (["conv3.batch_norm"], ["batch_norm"]):
        return True
    # GhostNet: ghost_module_2's primary BatchNorm and the shortcut conv's BatchNorm (ghostnet.py:134-140).
    if name.endswith(("ghost_module_2.primary_conv.batch_norm", "shortcut_conv.batch_norm")):
        return True
    return name.endswith(("bn3", "downsample.1", "conv2.batch_norm", "linear_conv.1")) or name.endswith(".bn2")


def fill(shapes, seed):
    """shapes: ordered {dotted name: shape}.  Returns {name: float32 array} by these rules:
      *.filters (conv OIHW)      N(0, sqrt(2/fan_in))
      *.weights (Linear in,out)  N(0, 0.02) clipped at 2 sigma         (vision_transformer.py:17)
      *.biases                   N(0, 0.02)
      *.gamma                    U(0.8, 1.2); U(0.2, 0.4) for the BN that feeds a residual add
      *.beta                     N(0, 0.05)
      *.moving_mean              N(0, 0.05)
      *.moving_var               U(0.8, 1.2)
      pos_embed / cls_token / relative_position_bias_table   N(0, 0.02) clipped at 2 sigma
      *_weight (attention projections, out x in)   N(0, sqrt(1/fan_in));   *_bias   N(0, 0.02)
      *.weight (1-D) / *.bias    the channels-first LayerNorm of ConvNeXt: as gamma / beta
      layer_scale_*              U(0.05, 0.15)                                   (VAN: van.py:139-143)
      attention_biases           N(0, 0.5)    LeViT's per-head bias by offset (levit.py:182): large enough that a wrong index moves logits
      patch_pos                  as pos_embed;  pixel_pos  N(0, 0.5): a wrong (c, ky, kx) order moves logits               (TNT: tnt.py:211-216)
      *attn_in.* / *mlp_in.* weights   N(0, fan_in^-1/2), x 1.5 for attn_in.qk: TNT's inner transformer (24 channels) would otherwise add
                                 O(0.01) a block and its softmax would be uniform, so a wrong inner kernel would move no logit
      blocks.<i>.<j>.attn.{q, kv, qkv, proj}.weights   Twins (gvt.py:52-56, :93-96): N(0, fan_in^-1/2), x 1.5 for q — for the same reason: at
                                 N(0, 0.02) the scores of both attentions would be O(0.01), every softmax uniform, and the attention half of
                                 a block would add O(0.01) to a stream of O(1); with these, 16 - 30 blocks add O(1) each and the stream
                                 stays far inside fp16.  `attn.sr.filters` takes the conv rule (fan_in = sr^2 C; a LayerNorm follows it)
      pos_block.<i>.proj.0.filters   Twins' PEG, a depthwise 3x3 added to its own input (gvt.py:311-325): N(0, fan_in^-1/2) = N(0, 1/3), so one
                                 PEG multiplies the stream's variance by 2, not by 3, and the four of them keep it far inside fp16
      pos_embeds.<i>             as pos_embed (gvt.py:240; PyramidVisionTransformer only: CPVTV2 deletes them)
      _ghostbottleneck_<i>.{ghost_module_2.*, depthwise_conv, shortcut_*}._conv.filters   GhostNet's convs that NO ReLU follows
                                 (ghostnet.py:109-126): N(0, fan_in^-1/2), not the ReLU gain sqrt(2) — up to four of them in a row, 16 blocks deep,
                                 would otherwise double the stream's variance each and leave fp16 (BatchNorm is an affine map in eval mode);
                                 with them, and the residual-feeding gamma rule on ghost_module_2.primary_conv / shortcut_conv, the stream stays O(10)
      features.{init_block.conv2, stage<i>.unit<j>}.conv2.*.filters   MixNet's projections (mixnet.py:410-417: a 1x1 conv, plain or in two
                                 groups, + BatchNorm with NO activation, added to the unit's input): N(0, fan_in^-1/2), not the ReLU gain
                                 sqrt(2).  Under the general rules the eval-mode stream grows about 1.3 x a unit (its BatchNorm gamma is
                                 named `conv2.bn`, which the residual-feeding gamma rule does not know) and peaks at 1254 (s), 1829 (m),
                                 7265 (l) with logits near 1000: outside fp16.  With this rule alone unit outputs stay between 1 and 36.
                                 The gamma is left at U(0.8, 1.2): a smaller gamma ON TOP of this rule kills the signal (the logits of two
                                 images then differ by 0.5 % of their range and share one argmax).  Keyed by names only MixNet has: the
                                 values drawn for every other model are unchanged
      bb_<b>_<i>.conv2.batch_norm.gamma   in a tree that has Res2Net's chain convs (bb_<b>_<i>.res<k><x>_branch2b_<s>: res2net.py:60-69) only:
                                 U(0.02, 0.06).  A Res2Net block is five convs deep (reduce, three chained 3x3, expand), each behind a ReLU, and
                                 under the residual-feeding rule U(0.2, 0.4) the pooled features of two images differ by 3 % after 16 blocks:
                                 the logits (range 90 - 130) of every seed tried share one argmax over the batch.  With the branch at
                                 U(0.02, 0.06) the stream stays below 30 and three seeds of eight give distinct, well separated classes.
                                 Same number of draws: the values drawn for every other model (ResNeXt's bb_<b>_<i>.conv2 included) are unchanged
      *.filters                  in a tree that has SqueezeNet's Fire modules (_conv<k>._conv_path1: squeezenet.py:37-46) only: drawn exactly as
                                 above, then every output channel's filter has its own mean subtracted.  SqueezeNet has no normalisation and
                                 every activation is non-negative, so under the general rule the features become a common mode: 23 of 24
                                 fixtures tried had one argmax on both rows, and such a fixture cannot tell a forward that ignores its input
                                 from a correct one.  With zero-mean filters 6 of 8 seeds (1.0) and 5 of 8 (1.1) give distinct, separated
                                 argmaxes, module outputs peak between 0.6 and 15 and the logit range is 0.1 - 0.3.  Same number of draws: the
                                 values drawn for every other model are unchanged
      dpn<k>.c1x1_c_func._conv.filters   in a tree that has DPN's DualPathFactories (dpn.py:103-105) only: drawn exactly as above, then scaled by
                                 DPN_C_GAIN = 0.6.  The first bw outputs of that conv are ADDED to the residual path, which no BatchNorm
                                 ever normalises (eval-mode BatchNorm is an affine map), and every block reads that path again: under the
                                 general rule the block states grow geometrically — DPN-68 at 96 x 160 peaks between 970 and 2280 over its 22
                                 blocks (7 of 8 seeds above the generator's limit of 1000), DPN-107 at 64 x 96 between 25 800 and 51 600 with
                                 logit ranges of 7 400 - 25 000: outside fp16.  With the gain DPN-68's states peak at 47 (224 x 224) and 78, DPN-107's
                                 at 314.  A smaller gain starves the image-dependent part of the features: at 0.25 and 0.5 the two rows of
                                 the batch-2 fixture share one argmax for all eight seeds.
                                 Same number of draws: the values drawn for every other model are unchanged
    """
    rng = np.random.default_rng(seed)
    res2net = any(_RES2NET_CHAIN.match(n) for n in shapes)
    squeezenet = any(_SQUEEZENET_FIRE.match(n) for n in shapes)
    dpn = any(_DPN_C.match(n) for n in shapes)
    out = {}
    for name, shape in shapes.items():
        shape = tuple(shape)
        leaf = name.rsplit(".", 1)[-1]
        owner = name.rsplit(".", 1)[0] if "." in name else ""
        if leaf == "filters" and owner.startswith("pos_block."):
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(1.0 / np.sqrt(np.prod(shape[1:])))
        elif leaf == "weights" and _TWINS_ATTN.match(owner):
            gain = 1.5 if owner.endswith(".q") else 1.0
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(gain / np.sqrt(shape[0]))
        elif owner == "pos_embeds":
            a = np.clip(rng.standard_normal(shape, dtype=np.float32), -2, 2) * np.float32(0.02)
        elif leaf == "filters" and _GHOST_LINEAR.match(owner):
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(1.0 / np.sqrt(np.prod(shape[1:])))
        elif leaf == "filters" and _MIXNET_PROJ.match(name):
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(1.0 / np.sqrt(np.prod(shape[1:])))
        elif leaf == "filters":
            fan_in = int(np.prod(shape[1:]))
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / fan_in))
            if squeezenet and a.size:
                a = a - a.reshape(shape[0], -1).mean(axis=1, dtype=np.float32).reshape((shape[0],) + (1,) * (len(shape) - 1))
            if dpn and _DPN_C.match(name):
                a = a * np.float32(DPN_C_GAIN)
        elif leaf == "weights" and ("attn_in." in owner + "." or "mlp_in." in owner + "."):      # TNT's inner transformer (tnt.py:125-129)
            gain = 1.5 if (owner + ".").endswith("attn_in.qk.") else 1.0
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(gain / np.sqrt(shape[0]))
        elif leaf == "weights":
            a = np.clip(rng.standard_normal(shape, dtype=np.float32), -2, 2) * np.float32(0.02)
        elif leaf == "biases":
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02)
        elif leaf == "gamma":
            lo, hi = (0.2, 0.4) if _is_last_bn_of_block(owner) else (0.8, 1.2)
            if res2net and _RES2NET_LAST_BN.match(owner):
                lo, hi = 0.02, 0.06
            a = rng.uniform(lo, hi, shape).astype(np.float32)
        elif leaf in ("beta", "moving_mean"):
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.05)
        elif leaf == "moving_var":
            a = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        elif leaf == "pixel_pos":                               # TNT (tnt.py:214-216): (1, in_dim, 4, 4)
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.5)
        elif leaf in ("pos_embed", "cls_token", "relative_position_bias_table", "absolute_pos_embed", "patch_pos"):
            a = np.clip(rng.standard_normal(shape, dtype=np.float32), -2, 2) * np.float32(0.02)
        elif leaf.endswith("_weight") and len(shape) == 2:      # attention projections stored (out, in): detr.py:975-995
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(1.0 / shape[1]))
        elif leaf.endswith("_bias"):
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02)
        elif leaf == "weight" and len(shape) == 1:              # ChannelsFirstLayerNorm (convnext.py:61-64): as gamma
            a = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        elif leaf == "bias":                                    # ... as beta
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.05)
        elif leaf.startswith("layer_scale_"):                   # VAN's [dim, 1, 1] layer scales (van.py:139-143): large enough to matter, small enough that 13 gated blocks stay far inside fp16
            a = rng.uniform(0.05, 0.15, shape).astype(np.float32)
        elif leaf == "attention_biases":                        # LeViT (levit.py:182-183, :284-285)
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.5)
        else:
            raise KeyError(f"seeded.fill: no rule for parameter {name!r}")
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


def shapes_of(module):
    """Ordered {name: shape} of a torch-style module's floating parameters and buffers."""
    derived = ("attn_mask", "relative_position_bias", "relative_position_index")   # computed, not learned
    return {k: tuple(v.shape) for k, v in module.state_dict().items()
            if v.is_floating_point() and k.rsplit(".", 1)[-1] not in derived}
