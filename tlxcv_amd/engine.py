"""Functional host layer over the C-ABI: torch tensors in, torch tensors out, HIP kernels inside.

PyTorch-ROCm is used here for device memory, streams and nothing else: every function below
hands `tensor.data_ptr()` and the current HIP stream to libtlxmi.so.  Activations are NHWC
(`(N, H, W, C)` contiguous, or `(rows, C)` token matrices); fp16 is the throughput dtype, fp32 the
parity dtype.  There is deliberately no CPU branch: a CPU tensor raises.
"""
import ctypes as C
import threading

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_HARDSIGMOID, ACT_HARDSWISH, ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_RELU6,
                   ACT_SIGMOID, ACT_SILU, EPI_RES_AFTER_ACT, F16, F32)

EPI_RES_BCAST_N = 2

_precision = torch.float16

# Host-side A/B switches (tools/ only; no environment variable is read on the product path).
_options = {"splitk": True,       # classifier heads: K slices side by side (tlxmi_linear_splitk)
            "attn_comb": True,    # Swin attention with the pre-summed bias + mask table (tlxmi_attention_comb)
            "seams": True,        # block-to-block seams of the bottleneck families as one launch (tlxmi_bottleneck_seam); off = the
                                  # expand conv and the next block's reduce conv as two launches (the A/B and the parity tests' other arm)
            "seam256": True,      # bottleneck seams with a 256-channel conv3 input (ResNet-50 layer3, 14 x 14) fused too
            "proj_fold": 7,       # (a bit mask) ResNet transition blocks (layer2.0 / layer3.0 / layer4.0 = bits 1 / 2 / 4): the 1x1 projection
                                  # shortcut as extra K of the block's expand conv (tlxmi_conv1x1_proj, fp16), its map neither written nor
                                  # read; a clear bit = the shortcut as its own launch, read back as the expand conv's residual (the A/B and
                                  # the parity tests' other arm).  All on: bits 1 and 2 each win alone; bit 4 is inside the noise
                                  # end to end but removes a launch and trades no seam for it (137 -> 84 us); mask 7 has the best mean (+1.9 .. 2.1 %)
            "seam_decimate": True,  # ResNet seams in front of a stage transition (layer1.2 -> layer2.0, layer2.3 -> layer3.0) store the block output
                                  # only at the pixels the next block's 1x1 stride-2 folded shortcut reads (tlxmi_bottleneck_seam_dec): a compact
                                  # (N, H/2, W/2, C) map, a quarter of the stores; off = the full map, read at stride 2 (the A/B and the tests' other arm)
            "two_streams": True,  # large batches as two half batches on two HIP streams (two_streams(), below)
            "conv_splitk": True,  # convs with few pixels and a long K on K slices (tlxmi_conv2d_splitk)
            "patch_linear": True, # ViT patch embedding as one Linear over all token rows (tlxmi_patchify + the persistent GEMM); off = the
                                  # space-to-depth implicit GEMM writing rows 1.. of each image (the A/B and the parity tests' other arm)
            "patch_embed4": True, # Swin patch embedding (conv 4 x 4 / 4 + LayerNorm) as one pass over the NCHW image (tlxmi_patch_embed4, fp16)
            "mlp_seam": True,     # Swin stage 1 (128 -> 512 -> 128): fc1 + GELU + fc2 + residual as one launch (tlxmi_mlp_seam), the hidden map stays on chip
            "lnfold": True,       # LayerNorm folded AROUND the Linear layers of a transformer block (fp16, round 5): proj / fc2 / the patch embedding
                                  # emit the row statistics of the residual stream from their epilogues (tlxmi_linear_stats), qkv / fc1 apply
                                  # the normalisation in theirs (tlxmi_linear_ln); off = LayerNorm launches + plain Linear layers (the parity
                                  # tests' other arm)
            "lnfold_min_rows": 2048,  # (a number) folded Linear layers need at least this many rows (below, the tiled kernels of the dispatcher win)
            "lnfold_min_rows_one_stream": 12000,  # (a number) ... and this many outside a two-stream forward
            "lnfold_min_c": 256,  # (a number) Swin: fold the LayerNorms of the stages with at least this many channels (tools/ A/B per stage)
            "sepconv": True,      # DeepLabV3+'s separable convs (fp16): depthwise 3x3 + BN -> pointwise 1x1 + BN + ReLU as one launch
                                  # (tlxmi_sepconv2d), the depthwise map kept on chip; off = tlxmi_dwconv2d then tlxmi_conv2d (the A/B and
                                  # the tests' other arm)
            "dwconv7": True,      # ConvNeXt's depthwise 7x7 (fp16) on tlxmi_dwconv7_stats: the input tile staged in LDS once, the taps in registers,
                                  # and the row statistics of the LayerNorm fold out of the same launch; off = tlxmi_dwconv2d (+ tlxmi_layernorm
                                  # in the model): the A/B and the tests' other arm
            "preact": True,       # DenseNet's pre-activation 1x1 convs (fp16): BatchNorm + ReLU of the INPUT applied on the way to the MFMA
                                  # (tlxmi_preact_conv1x1), the concat prefix read once; off = tlxmi_affine_act into a dense temporary then
                                  # tlxmi_conv2d (the A/B and the tests' other arm)
            "sr_attn": True,      # PVTv2's spatial-reduction attention (fp16, at most 64 keys, head dim 32 / 64) on tlxmi_sr_attention: K / V staged
                                  # once per workgroup, both products on MFMA, the scores in registers; off = tlxmi_mha, the general kernel
                                  # (the A/B and the tests' other arm)
            "lka": True,          # VAN's large-kernel attention (fp16): the depthwise 5x5 -> dilated 7x7 chain as one launch (tlxmi_lka_dw, the
                                  # intermediate map in LDS; planes of >= 196 pixels) and conv1 -> gate -> proj_2 -> layer scale + shortcut as one
                                  # launch (tlxmi_lka_gate, both products on MFMA, the gated map in registers; C <= 64); elsewhere and off = two tlxmi_dwconv2d launches, and tlxmi_conv2d -> tlxmi_mul
                                  # -> tlxmi_affine_act -> tlxmi_conv2d (the A/B and the tests' other arm)
            "cswin_attn": True,   # CSWin's cross-shaped window attention + LePE (fp16, head dim 32, stripes of at most 128 tokens) on
                                  # tlxmi_cswin_attention: K / V of a (stripe, head) staged once in LDS, both products on MFMA, the scores in
                                  # registers, LePE from the V tile in the epilogue; off = tlxmi_cswin_attention_plain (the A/B and the tests'
                                  # other arm)
            "levit_attn": True,   # LeViT's attention (fp16, keys 16 / 32 wide, values 32 / 64 / 128 wide, key grids up to 16 x 16, a bias per head
                                  # indexed by the distance on the key grid) on tlxmi_levit_attention: K / V / the bias table of an (image, head)
                                  # staged once in LDS, both products on MFMA, scores + bias + softmax in registers, Hardswish in the epilogue;
                                  # off = tlxmi_levit_attention_plain (the A/B and the tests' other arm)
            "tnt_inner": True,    # TNT's inner transformer block (fp16, 16 pixels x 24 channels a patch, 4 heads, hidden 96) on tlxmi_tnt_inner: three
                                  # LayerNorms, attention at head width 6 and the MLP in ONE launch, a wave per patch, the parameters staged once
                                  # per workgroup in LDS, every product on MFMA, the pixel map read once and written once; off =
                                  # tlxmi_tnt_inner_plain (the A/B and the tests' other arm)
            "gsa_block": True,    # Twins' GSA blocks of the wide stages (fp16, C 64 / 96 / 128, head dim 32 / 64, at most 64 reduced keys): norm1 ->
                                  # q Linear -> attention -> proj + residual on tlxmi_gsa_block: ONE launch, K / V of an image and both weights
                                  # staged in LDS, four chained MFMA products, the residual stream read once and written once; elsewhere and
                                  # off = tlxmi_layernorm -> tlxmi_conv2d -> tlxmi_sr_attention -> tlxmi_conv2d (the A/B and the tests' other arm)
            "shuffle_unit": True, # ShuffleNetV2's stride-1 units (fp16, half width h <= 128): split -> 1x1 + BN + act -> depthwise 3x3 + BN -> 1x1 + BN + act
                                  # -> concat -> channel_shuffle on tlxmi_shuffle_unit: ONE launch, both hidden maps in LDS, both products on MFMA,
                                  # the pixel read once and written once with the shuffle in the store; elsewhere and off = tlxmi_conv2d ->
                                  # tlxmi_dwconv2d -> tlxmi_conv2d -> tlxmi_shuffle_concat (the A/B and the tests' other arm)
            "ghost_module": True, # GhostNet's Ghost modules (fp16; the shapes the measured table keeps: maps up to 56 x 56, m <= 100, Cin * m <= 19200): 1x1 + BN + act -> depthwise 3x3 + BN + act -> concat
                                  # (+ the bottleneck's shortcut) on tlxmi_ghost_module: ONE launch, the primary map of a pixel tile in LDS, the
                                  # 1x1 on MFMA, both halves stored from the launch; off = tlxmi_conv2d -> tlxmi_dwconv2d (-> tlxmi_affine_act
                                  # for the shortcut) (the A/B and the tests' other arm)
            "mixconv": True,      # MixNet's mixed depthwise convs (fp16 and fp32; C a multiple of 8, up to five groups, odd windows 3 .. 11, stride 1 / 2):
                                  # split -> a depthwise conv a group, each with its own window -> concat -> BN + act, and the SE pool of the
                                  # result, on tlxmi_mixconv_dw: ONE launch, an 8-channel slab of an image (or of a row tile) in LDS, one read and
                                  # one write of the map; elsewhere and off = one tlxmi_dwconv2d a group (through dense copies where a group does
                                  # not start and end on 16-byte chunks) -> tlxmi_global_avgpool (the A/B and the tests' other arm)
            "res2chain": True,    # Res2Net's hierarchical 3x3 chain of a stride-1 block (fp16, 2 .. 8 slices of 8 .. 208 channels at a padded pitch; the
                                  # shapes the measured table keeps — the 56 x 56 blocks of 26w x 4s, the 56 x 56 and 28 x 28 ones of 14w x 8s:
                                  # engine.RES2_CHAIN_WINS):
                                  # conv -> add -> conv -> add -> conv -> copy on tlxmi_res2_chain: ONE launch, a band of rows of an image in LDS with
                                  # a halo that shrinks a row a conv, every 3x3 as nine MFMA taps, the map read once and written once; elsewhere
                                  # and off = tlxmi_conv2d -> tlxmi_affine_act (the add) -> tlxmi_conv2d ... -> tlxmi_copy_channels (the A/B and
                                  # the tests' other arm)
            "inception_head": True,  # GoogLeNet's Inception modules (fp16, widths multiples of 8; the shapes the measured table keeps:
                                  # engine.INCEPTION_HEAD_WINS — `_ince3a` alone as measured): the three 1x1 convs on x and maxpool 3/1/1 -> 1x1 conv on tlxmi_inception_head: ONE
                                  # launch, x staged once in LDS with a halo, the pooled tile an MFMA operand that never leaves the CU, the four
                                  # results written into their slices of the output map and of the mid map; elsewhere and off = tlxmi_conv2d x 3 ->
                                  # tlxmi_maxpool2d -> tlxmi_conv2d (the A/B and the tests' other arm)
            "fire_module": True,  # SqueezeNet's Fire modules (fp16, sq 16 / 32 / 48 / 64, widths multiples of 8; the shapes the measured table keeps:
                                  # engine.FIRE_MODULE_WINS): squeeze 1x1 -> expand 1x1 | expand 3x3 on tlxmi_fire_module: ONE launch, x read
                                  # once, the squeeze map of a haloed pixel tile in LDS only, both expands written into their slices of the output
                                  # map; elsewhere and off = tlxmi_conv2d x 3 with bias + ReLU epilogues (the A/B and the tests' other arm)
            "dual_path": True,    # DPN's `c` convs (fp16, widths multiples of 8; the shapes the measured table keeps: engine.DUAL_PATH_WINS,
                                  # DESIGN 4.33): the 1x1 conv whose output is split, added onto the residual path IN PLACE and appended to the
                                  # dense path of the stage buffer on tlxmi_dual_path_conv1x1: ONE launch, the operand read once; elsewhere and
                                  # off = tlxmi_conv2d twice on the two row ranges of the filter (the A/B and the tests' other arm)
            "link_conv": True,    # HarDNet's multi-link layers (fp16, R 1 or 3, up to 8 links, widths multiples of 8; the shapes the measured table
                                  # keeps: engine.LINK_CONV_WINS): the conv of a HarDBlock layer reads its linked layers as column
                                  # slices of the block buffer IN PLACE on tlxmi_link_conv2d: ONE launch, no concat pass; elsewhere and off = one
                                  # tlxmi_copy_channels a link into a scratch map, then tlxmi_conv2d (the A/B and the tests' other arm)
            "gated_conv": True,   # ReXNet's projecting 1x1 convs (fp16, widths and pitches multiples of 8; the shapes the measured table keeps:
                                  # engine.GATED_CONV_WINS): SE gate -> ReLU6 -> 1x1 conv + BN -> shortcut onto the first res_c channels
                                  # on tlxmi_gated_conv1x1: ONE launch, the gated map only on its way into the MFMA; elsewhere and off =
                                  # tlxmi_scale_channels -> tlxmi_affine_act -> tlxmi_conv2d with the shortcut as its residual (the A/B and the
                                  # tests' other arm)
            "tail_splitk": False} # Linear layers: the rows of a short last round of 256 x 256 tiles on K slices (_linear_tail): built,
                                  # parity-green, measured a LOSS on the ViT-B/16 forward (10.63 -> 11.61 ms for every K >= 768,
                                  # 10.91 for fc2 only: two more launches + the fp32 partial planes cost more than the idle round)


def set_option(name, value):
    if name not in _options:
        raise KeyError(f"unknown option {name!r}; have {sorted(_options)}")
    _options[name] = int(value) if isinstance(_options[name], int) and not isinstance(_options[name], bool) else bool(value)


def option_value(name):
    """A numeric option (set_option keeps the type the option was declared with)."""
    return _options[name]


def option(name):
    return _options[name]


# Optional per-launch probe (bench.py): when a list is installed, every implicit-GEMM launch appends
# (start_event, end_event, algorithmic_bytes, flops) recorded on the launch stream.
_probe = None


def set_probe(lst):
    global _probe
    _probe = lst


def set_precision(p):
    """'fp16' (throughput: fp16 storage, fp32 accumulate) or 'fp32' (parity: exact fp32)."""
    global _precision
    if p in ("fp16", "float16", torch.float16):
        _precision = torch.float16
    elif p in ("fp32", "float32", torch.float32):
        _precision = torch.float32
    else:
        raise ValueError(f"unknown precision {p!r}")


def precision():
    return _precision



def dt_code(dtype):
    if dtype == torch.float16:
        return F16
    if dtype == torch.float32:
        return F32
    raise RuntimeError(f"tlxcv_amd: unsupported dtype {dtype} (fp16 or fp32 only)")


def vec(dtype):
    return 8 if dtype == torch.float16 else 4


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def need_gpu(t, what="tensor"):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"tlxcv_amd: {what} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(
            f"tlxcv_amd: {what} lives on {t.device}; this engine only runs on an MI355X (HIP) device "
            "and has no CPU path — move the model and inputs to 'cuda'.")
    return t


def to_model_device(inputs, model):
    """Task-boundary upload: host tensors (or the {"images": ...} dict of the detectors, darknet.py:300) handed to a
    model that lives on the GPU are copied there — the reference scripts build their image on the host
    (predict.py:22-29).  A data transfer, not a compute path: a model that is itself on the CPU still raises."""
    p = next(model.parameters(), None)
    if p is None or not p.is_cuda:
        return inputs
    if isinstance(inputs, torch.Tensor):
        return inputs if inputs.is_cuda else inputs.to(p.device, non_blocking=True)
    if isinstance(inputs, dict):
        return {k: to_model_device(v, model) for k, v in inputs.items()}
    if isinstance(inputs, (list, tuple)):
        return type(inputs)(to_model_device(v, model) for v in inputs)
    return inputs


# Two half batches on two HIP streams.  A forward is a chain of launches that are each either MFMA-bound (3x3 convs, the
# Linear layers) or HBM-bound (1x1 convs with their skip, LayerNorm, window plumbing), one workgroup per CU for the big ones:
# every launch ends in a partly filled round while its successor waits.  With the batch cut in two and the halves on two
# streams the hardware fills those tails (and overlaps launches of different kind) with the other half's workgroups: measured,
# hipGraph replay, ResNet-50 batch 256 3.77 -> 3.52 ms (batch 512 7.11 -> 6.43, batch 128 2.17 -> 2.12, batch 64 -1 %), Swin-B
# batch 128 9.14 -> 8.60 ms, VGG-16 batch 64 2.75 -> 2.63 ms, ViT-B/16 batch 256 unchanged (not applied there).  The halves are
# independent (eval-mode forward, no batch statistics): the result is the concatenation, row for row what the halves give alone.
_cache_builds = 0
# Per host THREAD: whether a two-stream forward is being enqueued and which planning hint its launches carry
# (TLXMI_PLAN_SHARED_* in every conv / linear descriptor).  Nothing process-wide is mutated: two threads — or two models —
# may enqueue forwards at the same time without changing each other's tile choices.
_tls = threading.local()


def in_halves():
    """True while a two-stream forward is being enqueued (launch-shape choices that count on the other stream's launches)."""
    return getattr(_tls, "depth", 0) > 0


def plan_flags():
    """Planning bits for the descriptors of the launches enqueued by this thread right now."""
    return getattr(_tls, "plan", 0)


class shared_plan:
    """with shared_plan("half" | "full" | None): the conv / linear launches enqueued by this thread carry TLXMI_PLAN_SHARED_*."""

    def __init__(self, plan):
        self.bits = {"half": _lib.PLAN_SHARED_HALF, "full": _lib.PLAN_SHARED_FULL, None: 0}[plan]

    def __enter__(self):
        self.prev = getattr(_tls, "plan", 0)
        _tls.plan = self.bits
        return self

    def __exit__(self, *exc):
        _tls.plan = self.prev
        return False


def note_cache_build():
    """A layer built a derived tensor (packed filter, folded BatchNorm, bias / mask table) just now, on the current stream.
    Not while a hipGraph is being captured: the build (and the redo of the two-stream forward it triggers) would be recorded
    into the graph for good — run one eager forward first (bench.py, graph.GraphedForward and the tests do)."""
    global _cache_builds
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("tlxcv_amd: a layer built its packed filter / folded BatchNorm / table during hipGraph capture; "
                           "run one eager forward of the model (same precision, same weights) before capturing")
    _cache_builds += 1


def run_halves(fn, x, plan=None):
    """fn(first half) on the current stream, fn(second half) on the device's side stream, joined; returns the concatenation.
    Derived tensors are built lazily on whichever stream asks first, and the other stream would read them unordered: when a
    build happened during the call (first forward, new weights, new precision) the streams are joined and the two halves are
    done again — the same launches every later call makes, so the first result equals the later ones bit for bit.
    plan: while the halves are enqueued every conv / linear descriptor carries a planning hint (TLXMI_PLAN_SHARED_*: the
    launch shares the device) — "half": tiles priced for half the CUs and no tail splits (ResNet-50 batch 256 -3 %; Swin-B
    +3 %), "full": the device's CU count, no tail splits only (Swin-B batch 128 -1.3 %).  The hint is per call, the side stream
    and the bookkeeping per host thread.  What IS process-wide: the count of derived-tensor builds — two threads that share ONE
    model must not race its first forward (run it once on one thread first); separate models per thread are independent."""
    cur = torch.cuda.current_stream(x.device)
    idx = x.device.index if x.device.index is not None else torch.cuda.current_device()
    sides = getattr(_tls, "side_streams", None)      # per host thread AND device: two threads forwarding on one GPU do not
    if sides is None:                                # serialise through one shared side stream
        sides = _tls.side_streams = {}
    side = sides.get(idx)
    if side is None:
        side = sides[idx] = torch.cuda.Stream(device=x.device)
    n = x.shape[0] // 2
    _tls.depth = getattr(_tls, "depth", 0) + 1
    hint = shared_plan(plan)
    hint.__enter__()
    try:
        for _ in range(3):
            builds = _cache_builds
            side.wait_stream(cur)                 # x is ready for the side stream (and: a redo starts after everything before it)
            y0 = fn(x[:n])                        # (first: lazy builds land on the caller's stream)
            with torch.cuda.stream(side):
                y1 = fn(x[n:])
            cur.wait_stream(side)
            if _cache_builds == builds:
                y1.record_stream(cur)
                return torch.cat((y0, y1), 0)
    finally:
        _tls.depth -= 1
        hint.__exit__()
    return fn(x)


# Every kernel addresses a tensor through 32-bit buffer offsets: no activation operand of a launch may reach this many bytes
# ("Sizing").  two_streams() cuts a forward's batch into chunks that stay below it.
ACT_LIMIT = 1 << 31


class _Oversize(Exception):
    """Raised by _note_act() inside a sizing forward at the first operand of ACT_LIMIT bytes or more (before its launch)."""


def _note_act(*nbytes):
    """The largest activation operand (x / y / residual bytes of a launch) of the forward being sized by two_streams()."""
    m = max(nbytes)
    if m >= ACT_LIMIT:
        raise _Oversize()
    if m > _tls.act_max:
        _tls.act_max = m


def _sizing():
    """True inside a sizing forward (_sized()): a launch then reports its operand bytes to _note_act().  The byte arguments stay behind
    this guard: an eager forward outside it pays one attribute lookup per launch and no numel() products."""
    return getattr(_tls, "act_max", None) is not None


def _timed(launch, entry):
    """launch() -> its result.  With a probe list installed, one (start_event, end_event, bytes, flops, label) entry is recorded around
    it; entry() -> (bytes, flops, label) is evaluated after the launch.  The list is taken away meanwhile, so engine calls inside
    launch() record nothing (a chain of launches is one entry); if launch() raises nothing is appended and the list is put back."""
    global _probe
    if _probe is None:
        return launch()
    probe, _probe = _probe, None
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = launch()
        e1.record()
    finally:
        _probe = probe
    probe.append((e0, e1, *entry()))
    return res


def _use_fused(op, fused, takes, default, describe):
    """The fused=None / True / False argument of a two-arm op -> whether tlxmi_<op> runs.  None: `default` (the option, the routing
    table and the library's predicate, in the order the op asks them); True: raises where the library does not take the call
    (`takes`; describe() names the operands); False: the layered arm.  takes / default: values, or callables asked only when needed."""
    if fused is None:
        return bool(default() if callable(default) else default)
    if fused and not (takes() if callable(takes) else takes):
        raise RuntimeError(f"{op}: tlxmi_{op} does not take {describe()}")
    return bool(fused)


def _out_map(op, out, N, H, W, min_c, dtype, device, default_ld, multiple=1, what=""):
    """The output of a fused op: `out`, or a new (N, H, W, default_ld) map -> (out, its pixel pitch).  A dense NHWC map of that dtype
    and those pixels whose last axis, the pitch, holds at least min_c channels and is a multiple of `multiple`; else "out must be <what>"."""
    if out is None:
        out = torch.empty((N, H, W, default_ld), dtype=dtype, device=device)
    y_ld = out.shape[-1]
    if out.dtype != dtype or tuple(out.shape[:3]) != (N, H, W) or y_ld < min_c or y_ld % multiple or not out.is_contiguous():
        raise RuntimeError(f"{op}: out must be {what}")
    return out, y_ld


def image_bytes(model, x):
    """Bytes per image of the largest activation operand of model's forward on inputs shaped like x (at the current precision),
    or None while it has not been measured (the first eager forward of that shape measures it; see two_streams())."""
    return vars(model).get("_act_bytes_per_image", {}).get((tuple(x.shape[1:]), x.dtype, precision()))


def chunk_sizes(batch, per_image):
    """Near-equal chunks of `batch` images whose largest activation operand stays below ACT_LIMIT ([batch] when one fits)."""
    if not per_image or batch * per_image < ACT_LIMIT:
        return [batch]
    cap = (ACT_LIMIT - 1) // per_image
    if cap < 1:
        raise RuntimeError(f"tlxcv_amd: one image needs a tensor of {per_image} bytes, beyond the 2 GiB the kernels address")
    k = -(-batch // cap)
    n, r = divmod(batch, k)
    return [n + 1] * r + [n] * (k - r)


def _sized(run, x, images):
    """run(x) while recording its largest activation operand -> (run(x), bytes per image), `images` = the images of one launch;
    (None, None) when an operand reached ACT_LIMIT (nothing of that size was launched)."""
    _tls.act_max = 0
    try:
        y = run(x)
        return y, -(-_tls.act_max // images)
    except _Oversize:
        torch.cuda.synchronize()          # what was enqueued before the refusal (on either stream) is finished and dropped
        return None, None
    finally:
        _tls.act_max = None


def two_streams(min_batch, plan=None, eager=True):
    """Decorator of a model's forward(self, x).
    First the batch is cut into chunk_sizes() chunks: one, unless some activation operand of the forward would reach ACT_LIMIT
    bytes.  The bytes per image are measured on the first eager forward of an input shape and kept on the model per (input shape,
    dtype, precision) — a hipGraph capture, which needs that eager forward first, reuses them; a first forward that reaches the limit
    stops before that launch and is sized on one image instead.  Then each chunk of at least `min_batch` (even) images runs as
    run_halves(), and the logits of the chunks are joined.
    plan: None / "half" / "full" (run_halves), or a callable batch -> one of these.
    eager=False: halves only while a hipGraph is being captured.  A forward of many tiny launches (MobileNetV3, EfficientNet: 150 - 250
    kernels of a few microseconds) is bound by the host when launched kernel by kernel, and two halves are twice the host work
    (MobileNetV3-small batch 256: 1.4 -> 2.3 ms eager, 1.37 -> 1.25 ms as a graph)."""
    def deco(fwd):
        import functools

        def split(x):
            return (_options["two_streams"] and x.shape[0] >= min_batch and x.shape[0] % 2 == 0 and _probe is None
                    and (eager or torch.cuda.is_current_stream_capturing()))

        def halves(self, x):
            if split(x):
                return run_halves(lambda h: fwd(self, h), x, plan(x.shape[0]) if callable(plan) else plan)
            return fwd(self, x)

        @functools.wraps(fwd)
        def wrapper(self, x, *args, **kwargs):
            if args or kwargs or not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4):
                return fwd(self, x, *args, **kwargs)
            if _sizing():      # inside the sizing forward of an enclosing model
                return fwd(self, x)
            key = (tuple(x.shape[1:]), x.dtype, precision())
            per = image_bytes(self, x)
            if per is None and not torch.cuda.is_current_stream_capturing():
                y, per = _sized(lambda h: halves(self, h), x, x.shape[0] // 2 if split(x) else x.shape[0])
                if per is None:
                    _, per = _sized(lambda h: fwd(self, h), x[:1], 1)
                    if per is None:
                        raise RuntimeError("tlxcv_amd: one image of this forward needs a tensor beyond the 2 GiB the kernels address")
                vars(self).setdefault("_act_bytes_per_image", {})[key] = per
                if y is not None:
                    return y
            sizes = chunk_sizes(x.shape[0], per)
            if len(sizes) == 1:
                return halves(self, x)
            return torch.cat([halves(self, c) for c in torch.split(x, sizes, 0)], 0)
        return wrapper
    return deco


def _f32(t):
    if t is None:
        return None
    need_gpu(t, "parameter")
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.detach().to(torch.float32).contiguous()
    return t.detach()


# ---------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------
def nchw_to_nhwc(x, dtype=None, cpad=None):
    """(N,C,H,W) contiguous -> (N,H,W,Cpad) `dtype`; extra channels are zero."""
    need_gpu(x, "input")
    dtype = dtype or _precision
    N, Cc, H, W = x.shape
    v = vec(dtype)
    cpad = cpad or (Cc + v - 1) // v * v
    if x.dtype not in (torch.float16, torch.float32):
        x = x.float()
    x = x.contiguous()
    y = torch.empty((N, H, W, cpad), dtype=dtype, device=x.device)
    _lib.call("tlxmi_nchw_to_nhwc", _p(x), dt_code(x.dtype), _p(y), dt_code(dtype), N, Cc, H, W, cpad, _stream())
    return y


def nchw_to_nhwc_s2d(x, b, dtype=None):
    """(N,C,H,W) -> (N,H/b,W/b,pad(b*b*C)): b x b space-to-depth fold, channel (ph*b+pw)*C + c."""
    need_gpu(x, "input")
    dtype = dtype or _precision
    N, Cc, H, W = x.shape
    if H % b or W % b:
        raise RuntimeError(f"space-to-depth needs H, W multiples of {b}, got {H}x{W}")
    v = vec(dtype)
    cpad = (b * b * Cc + v - 1) // v * v
    if x.dtype not in (torch.float16, torch.float32):
        x = x.float()
    x = x.contiguous()
    y = torch.empty((N, H // b, W // b, cpad), dtype=dtype, device=x.device)
    _lib.call("tlxmi_nchw_to_nhwc_s2d", _p(x), dt_code(x.dtype), _p(y), dt_code(dtype), N, Cc, H, W, b, cpad, _stream())
    return y


def patchify(x, ps, lead=0, dtype=None):
    """(N,C,H,W) -> (N, lead + (H/ps)(W/ps), C*ps*ps) patch rows in the order of the flattened conv filter [Cout][C][ps][ps]; the `lead`
    rows in front of each image's patches are zero (tlxmi_patchify)."""
    need_gpu(x, "input")
    dtype = dtype or _precision
    N, Cc, H, W = x.shape
    if ps % 8 or H % ps or W % ps:
        raise RuntimeError(f"patchify needs a patch size that is a multiple of 8 and divides H, W; got {ps} on {H}x{W}")
    if x.dtype not in (torch.float16, torch.float32):
        x = x.float()
    x = x.contiguous()
    y = torch.empty((N, lead + (H // ps) * (W // ps), Cc * ps * ps), dtype=dtype, device=x.device)
    _lib.call("tlxmi_patchify", _p(x), dt_code(x.dtype), _p(y), dt_code(dtype), N, Cc, H, W, ps, lead, _stream())
    return y


def patch_embed4_filter(w_oihw):
    """Conv filter (D, 3, 4, 4) -> the (D, 64) fp16 image tlxmi_patch_embed4 reads: k = 16 c + 4 ky + kx, zeros above 48."""
    w = _f32(w_oihw)
    D = w.shape[0]
    out = torch.zeros((D, 64), dtype=torch.float16, device=w.device)
    out[:, :48] = w.reshape(D, 48).to(torch.float16)
    return out


def patch_embed4(x, w64, bias, gamma, beta, eps, pos=None):
    """(N,3,H,W) fp32 / fp16 -> (N, H/4 * W/4, D) fp16 = LayerNorm(conv4x4/4(x) + bias) (no LayerNorm when gamma is None) [+ pos, the
    (H/4 * W/4, D) absolute position embedding of SwinTransformer(ape=True)], one pass."""
    need_gpu(x, "input")
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 4 or x.shape[3] % 4:
        raise RuntimeError(f"patch_embed4: a (N, 3, H, W) image with H, W multiples of 4 is expected, got {tuple(x.shape)} (the kernel reads 3 colour planes)")
    if w64.dim() != 2 or w64.shape[1] != 64 or w64.dtype != torch.float16:
        raise RuntimeError("patch_embed4: the filter must be the (D, 64) fp16 image of patch_embed4_filter()")
    if (gamma is None) != (beta is None):
        raise RuntimeError("patch_embed4: gamma and beta go together (both None: no LayerNorm)")
    if x.dtype not in (torch.float16, torch.float32):
        x = x.float()
    x = x.contiguous()
    N, Cc, H, W = x.shape
    D = w64.shape[0]
    y = torch.empty((N, (H // 4) * (W // 4), D), dtype=torch.float16, device=x.device)
    if pos is not None:
        pos = _f32(pos).reshape(-1, D).contiguous()
        if pos.shape[0] != (H // 4) * (W // 4):
            raise RuntimeError(f"patch_embed4: position table of {pos.shape[0]} rows for {(H // 4) * (W // 4)} tokens")
        _lib.call("tlxmi_patch_embed4_pos", _p(x), dt_code(x.dtype), _p(w64), _p(_f32(bias)), _p(_f32(gamma)), _p(_f32(beta)), _p(pos), _p(y), N, H, W, D,
                  C.c_float(eps), _stream())
        return y
    _lib.call("tlxmi_patch_embed4", _p(x), dt_code(x.dtype), _p(w64), _p(_f32(bias)), _p(_f32(gamma)), _p(_f32(beta)), _p(y), N, H, W, D,
              C.c_float(eps), _stream())
    return y


_resample_tables = {}


def _resample_table(n_in, n_out, interpolation, device):
    key = (n_in, n_out, interpolation, str(device))
    if key not in _resample_tables:
        import numpy as np
        from .tlx.vision.transforms import resample
        if n_in == n_out:       # PIL skips the pass: identity table
            b = np.stack([np.arange(n_out, dtype=np.int32), np.ones(n_out, dtype=np.int32)], 1)
            k = np.full((n_out, 1), 1 << resample.PRECISION_BITS, dtype=np.int32)
        else:
            b, k = resample.coefficients(n_in, n_out, interpolation)
        _resample_tables[key] = (torch.from_numpy(np.ascontiguousarray(b)).to(device), torch.from_numpy(np.ascontiguousarray(k)).to(device), k.shape[1])
    return _resample_tables[key]


def preprocess_u8(images, size, mean=None, std=None, layout="CHW", dtype=torch.float32, interpolation="bilinear", fold=0):
    """uint8 HWC images (N,H,W,C) on the device -> Resize(size) -> Normalize(mean, std) (or /255 without) -> ToTensor,
    one call (tlxmi_preprocess_u8), bit-identical to the host pipeline of tlx.vision.transforms.  layout 'CHW' -> (N,C,h,w),
    'HWC' -> (N,h,w,C); fold=b -> the b x b space-to-depth NHWC image the stem kernels read ((N,h/b,w/b,pad(b*b*C)))."""
    from .tlx.vision.transforms import resample
    if interpolation not in resample.SUPPORTED:
        raise RuntimeError(f"preprocess_u8: interpolation {interpolation!r} is not supported (supported: {', '.join(resample.SUPPORTED)})")
    need_gpu(images, "images")
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise RuntimeError("preprocess_u8: a (N, H, W, C) uint8 tensor is expected")
    images = images.contiguous()
    N, H, W, Cc = images.shape
    oh, ow = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    xb, xk, kw = _resample_table(W, ow, interpolation, images.device)
    yb, yk, kh = _resample_table(H, oh, interpolation, images.device)
    norm = mean is not None
    def per_channel(v):      # a scalar or length-1 mean / std broadcasts over the channels, as on the host (numpy)
        t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
        if t.numel() == 1 and Cc > 1:
            t = t.expand(Cc)
        return t.to(images.device).contiguous()
    m = per_channel(mean) if norm else None
    sd = per_channel(std if std is not None else 1.0) if norm else None
    if norm and (m.numel() != Cc or sd.numel() != Cc):
        raise RuntimeError(f"preprocess_u8: mean / std must have 1 or {Cc} entries")
    if fold:
        v = vec(dtype)
        cpad = (fold * fold * Cc + v - 1) // v * v
        out = torch.empty((N, oh // fold, ow // fold, cpad), dtype=dtype, device=images.device)
        lay = 2
    elif layout == "CHW":
        out, lay, cpad = torch.empty((N, Cc, oh, ow), dtype=dtype, device=images.device), 0, 0
    elif layout == "HWC":
        out, lay, cpad = torch.empty((N, oh, ow, Cc), dtype=dtype, device=images.device), 1, 0
    else:
        raise ValueError("layout should be CHW or HWC")
    d = _lib.PreprocDesc(N=N, H=H, W=W, C=Cc, out_h=oh, out_w=ow, kh=kh, kw=kw, out_dtype=dt_code(dtype), layout=lay, fold_b=int(fold),
                         cpad=cpad, normalize=1 if norm else 0)
    ws = torch.empty(_lib.load().tlxmi_preprocess_u8_workspace_bytes(C.byref(d)), dtype=torch.uint8, device=images.device)
    _lib.call("tlxmi_preprocess_u8", C.byref(d), _p(images), _p(xb), _p(xk), _p(yb), _p(yk), _p(m), _p(sd), _p(ws), _p(out), _stream())
    return out


def s2d_filter(w_oihw, b, pad):
    """Re-index an OIHW filter for a b x b space-to-depth input (host side, once):
    W2[o][(ph*b+pw)*C + c][r2][s2] = W[o][c][b*r2 + ph - off][b*s2 + pw - off], zero outside;
    returns (W2, new padding).  The conv then runs with stride/b and output extent cropped by the caller."""
    O, Cc, R, S = w_oihw.shape
    ph_ = pad if isinstance(pad, int) else pad[0]
    pad2 = (ph_ + b - 1) // b
    off = pad2 * b - ph_
    R2, S2 = (R + off + b - 1) // b, (S + off + b - 1) // b
    w2 = torch.zeros((O, b * b * Cc, R2, S2), dtype=torch.float32, device=w_oihw.device)
    w = w_oihw.detach().float()
    for ph in range(b):
        for pw in range(b):
            for r2 in range(R2):
                r = b * r2 + ph - off
                if not 0 <= r < R:
                    continue
                for s2 in range(S2):
                    sx = b * s2 + pw - off
                    if 0 <= sx < S:
                        w2[:, (ph * b + pw) * Cc:(ph * b + pw + 1) * Cc, r2, s2] = w[:, :, r, sx]
    return w2, pad2


def nhwc_to_nchw(x, C_true=None, dtype=None):
    """(N,H,W,ld) -> contiguous (N,C,H,W)."""
    need_gpu(x)
    N, H, W, ld = x.shape
    Cc = C_true or ld
    dtype = dtype or x.dtype
    y = torch.empty((N, Cc, H, W), dtype=dtype, device=x.device)
    _lib.call("tlxmi_nhwc_to_nchw", _p(x), dt_code(x.dtype), ld, _p(y), dt_code(dtype), N, Cc, H, W, _stream())
    return y


# ---------------------------------------------------------------------------------------------
# filters / batch-norm folding
# ---------------------------------------------------------------------------------------------
class PackedFilter:
    """A conv / linear weight in the K-contiguous, padded image tlxmi_conv2d reads."""

    def __init__(self, w_oihw, dtype):
        w = _f32(w_oihw)
        if w.dim() == 2:  # Linear weight [out, in]
            w = w.reshape(w.shape[0], w.shape[1], 1, 1)
        self.Cout, self.Cin, self.R, self.S = w.shape
        self.dtype = dtype
        v = vec(dtype)
        self.Cin_pad = (self.Cin + v - 1) // v * v
        nbytes = _lib.load().tlxmi_packed_filter_bytes(self.Cout, self.Cin, self.R, self.S, dt_code(dtype))
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        _lib.call("tlxmi_pack_filter", _p(w), _p(self.buf), self.Cout, self.Cin, self.R, self.S, dt_code(dtype),
                  _stream())


class PackedGroupFilter:
    """Filter of a grouped convolution (1 < groups < C, resnext.py:30-40): `chunks` block-diagonal packed filters,
    one per launch chunk of tlxmi_group_conv2d."""

    def __init__(self, w_oihw, groups, dtype):
        w = _f32(w_oihw)
        self.Cout, cg, self.R, self.S = w.shape
        self.groups = int(groups)
        self.Cin = cg * self.groups
        self.Cin_pad = self.Cin
        self.dtype = dtype
        lib = _lib.load()
        self.chunks = lib.tlxmi_group_conv_chunks(self.Cin, self.Cout, self.groups, dt_code(dtype))
        if self.chunks <= 0:
            raise NotImplementedError(f"grouped conv {self.Cin}->{self.Cout} in {self.groups} groups: channel counts "
                                      "cannot be merged into 16-byte aligned launch chunks")
        nbytes = lib.tlxmi_packed_group_filter_bytes(self.Cout, self.Cin, self.R, self.S, self.groups, dt_code(dtype))
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        _lib.call("tlxmi_pack_group_filter", _p(w), _p(self.buf), self.Cout, self.Cin, self.R, self.S, self.groups,
                  dt_code(dtype), _stream())


def _round_up(n, k):
    return (int(n) + k - 1) // k * k


def _zero_padded(t, shape, dtype, device=None):
    """Zeros of `shape` / `dtype` with t converted and written into the leading corner, on `device` (default: t's).  t: a tensor, or a
    sequence of equal tensors that become the rows of a new leading axis."""
    if not isinstance(t, torch.Tensor):
        device = device or t[0].device
        t = torch.stack([v.detach().to(device=device, dtype=dtype) for v in t])
    out = torch.zeros(shape, dtype=dtype, device=device or t.device)
    out[tuple(slice(0, n) for n in t.shape)] = t.detach().to(dtype)
    return out


def _dw_rsc(wdw, n_pad, dtype, device=None):
    """A depthwise filter (n, 1, k, k) -> [k][k][n_pad] in `dtype`, the channels behind n zero: what tlxmi_dwconv2d reads; reshaped to
    (k * k, n_pad) its rows are the taps r * k + s of the parameter images."""
    k = int(wdw.shape[-1])
    return _zero_padded(wdw.detach()[:, 0].permute(1, 2, 0), (k, k, n_pad), dtype, device)


def _param_image(*tensors):
    """Dense tensors of any dtype, one behind the other, as the one uint8 buffer a fused kernel stages."""
    return torch.cat([t.contiguous().view(torch.uint8).reshape(-1) for t in tensors])


def fold_bn(gamma, beta, mean, var, eps, conv_bias=None):
    """Eval-mode BatchNorm (+ optional conv bias) -> per-channel fp32 (scale, shift)."""
    ref = next(t for t in (gamma, beta, mean, var, conv_bias) if t is not None)
    Cn = ref.numel()
    g, b, m, v, cb = (_f32(t) for t in (gamma, beta, mean, var, conv_bias))
    scale = torch.empty(Cn, dtype=torch.float32, device=ref.device)
    shift = torch.empty(Cn, dtype=torch.float32, device=ref.device)
    _lib.call("tlxmi_fold_bn", _p(g), _p(b), _p(m), _p(v), _p(cb), float(eps), Cn, _p(scale), _p(shift), _stream())
    return scale, shift


# ---------------------------------------------------------------------------------------------
# conv / linear
# ---------------------------------------------------------------------------------------------
_cus = {}


def _pair(v):
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def conv2d(x, pk, stride=1, padding=0, dilation=1, scale=None, shift=None, res=None, act=ACT_NONE,
           act_param=0.0, res_after_act=False, out=None, out_ld=None, y_nstride=0, res_nstride=0,
           res_bcast=False, res_ld=None, out_hw=None, overhang=False, maxpool3s2=False, x_ld=None):
    """x (N,H,W,C>=Cin_pad...) NHWC -> y (N,Ho,Wo,Cout).  `out` may be a wider/pre-offset buffer.
    maxpool3s2: fold nn.MaxPool2d(3, 2, 1) into the conv's epilogue (TLXMI_EPI_MAXPOOL_3S2P1) -> (N,Ho/2,Wo/2,Cout);
    returns None — nothing launched — when the library has no fused kernel for this geometry.
    x_ld: the pixel pitch when x is a 16-byte aligned column slice of a wider map (a view: its last axis is the slice's width)."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    if x_ld is not None:
        if x_ld < ld or pk.Cin_pad > ld:
            raise RuntimeError(f"conv2d: a column slice of {ld} channels at pitch {x_ld} cannot feed a filter of {pk.Cin_pad}")
        ld = int(x_ld)
    if x.dtype != pk.dtype:
        raise RuntimeError(f"conv2d: input dtype {x.dtype} != packed filter dtype {pk.dtype}")
    if ld < pk.Cin_pad:
        raise RuntimeError(f"conv2d: input has {ld} channels, filter expects {pk.Cin} (padded {pk.Cin_pad})")
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dh, dw = _pair(dilation)
    Ho = (H + 2 * ph - dh * (pk.R - 1) - 1) // sh + 1
    Wo = (W + 2 * pw - dw * (pk.S - 1) - 1) // sw + 1
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError(f"conv2d: empty output {Ho}x{Wo} for input {H}x{W}")
    if out_hw is not None:      # crop (asymmetric padding of a space-to-depth stem), or one-sided end padding ('SAME' at stride 2)
        Ho, Wo = (int(out_hw[0]), int(out_hw[1])) if overhang else (min(Ho, out_hw[0]), min(Wo, out_hw[1]))
    if maxpool3s2 and (out is not None or res is not None):
        return None
    if out is None:
        out = None if maxpool3s2 else torch.empty((N, Ho, Wo, pk.Cout), dtype=x.dtype, device=x.device)
        out_ld = pk.Cout
    elif out_ld is None:
        out_ld = out.shape[-1]
    d = _lib.ConvDesc(dtype=dt_code(x.dtype), N=N, H=H, W=W, C=pk.Cin_pad, Cout=pk.Cout, R=pk.R, S=pk.S,
                      stride_h=sh, stride_w=sw, pad_h=ph, pad_w=pw, dil_h=dh, dil_w=dw, Ho=Ho, Wo=Wo,
                      x_ld=ld, y_ld=out_ld, res_ld=(res_ld if res_ld is not None else (res.shape[-1] if res is not None else 0)),
                      y_nstride=y_nstride, res_nstride=res_nstride, act=act, act_param=float(act_param),
                      flags=(EPI_RES_AFTER_ACT if res_after_act else 0) | (EPI_RES_BCAST_N if res_bcast else 0)
                      | (_lib.EPI_MAXPOOL_3S2P1 if maxpool3s2 else 0) | plan_flags())
    if res is not None and res.dtype != x.dtype:
        raise RuntimeError("conv2d: residual dtype mismatch")
    if maxpool3s2:
        if not _lib.load().tlxmi_conv2d_maxpool_supported(C.byref(d)):
            return None
        out = torch.empty((N, Ho // 2, Wo // 2, pk.Cout), dtype=x.dtype, device=x.device)
    M = N * Ho * Wo
    if _sizing():
        _note_act(x.numel() * x.element_size(), M * out_ld * x.element_size(), M * d.res_ld * x.element_size() if res is not None else 0)
    splits = 0 if maxpool3s2 else _conv_splits(d, M, pk, x, out_ld, y_nstride, res_nstride, res_bcast)

    def launch():
        if splits:
            # few output pixels, long K (the 7 x 7 stage of a ResNet, small batches): K slices side by side + a reduction
            part = torch.empty((splits, M, pk.Cout), dtype=torch.float32, device=x.device)
            _lib.call("tlxmi_conv2d_splitk", C.byref(d), splits, _p(x), _p(pk.buf), _p(part), _p(scale), _p(shift), _p(res), _p(out), _stream())
        else:
            _lib.call("tlxmi_conv2d", C.byref(d), _p(x), _p(pk.buf), _p(scale), _p(shift), _p(res), _p(out), _stream())
    if _probe is None:      # 60 - 100 of a small model's launches come through here: the host-bound forwards (two_streams()) pay neither the
        launch()            # helper's call nor the entry's closure (measured: 0.5 - 1 % of MobileNetV3-small's eager forward)
        return out
    _timed(launch, lambda: ((N * H * W * pk.Cin + (M // 4 if maxpool3s2 else M) * pk.Cout * (2 if res is not None else 1)
                             + pk.Cout * pk.Cin * pk.R * pk.S) * x.element_size(), 2 * M * pk.Cout * pk.Cin * pk.R * pk.S,
                            (N, H, W, pk.Cin, pk.Cout, pk.R, sh, res is not None)))
    return out


def _conv_splits(d, M, pk, x, out_ld, y_nstride, res_nstride, res_bcast):
    """Number of K slices for a convolution whose few tiles each walk a long K in sequence while most CUs idle (0: one launch).
    The slices cost a second launch (the reduction) and the partial planes, ~20 us: measured (tools/splitk_conv_check.py) the
    3x3 512 -> 512 convs of ResNet's 7 x 7 stage win up to 32 images (26 tiles x 72 K tiles: 46.9 -> 32.5 us in 8 slices; 4 images
    32.8 -> 26.7) and lose from 128 (98 tiles: 53.7 -> 64.2 us); 36 K tiles (14 x 14, 256 channels) lose at any batch.
    set_option("conv_splitk", False) turns the path off (A/B)."""
    if not _options["conv_splitk"] or y_nstride or res_nstride or res_bcast or out_ld != pk.Cout or pk.Cout < 128:
        return 0
    if not (pk.S == 3 or (pk.R == 1 and pk.S == 1 and (d.stride_h > 1 or d.stride_w > 1))):
        return 0
    es = x.element_size()
    ktiles = pk.R * pk.S * pk.Cin_pad * es // 128
    if ktiles < 64:
        return 0
    idx = x.device.index if x.device.index is not None else torch.cuda.current_device()
    if idx not in _cus:
        _cus[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    tiles = ((M + 127) // 128) * ((pk.Cout + 255) // 256)
    if tiles * 8 > _cus[idx]:
        return 0
    s_ = min(8, _cus[idx] // max(tiles, 1), ktiles // 8)
    if s_ < 2:
        return 0
    return s_ if _lib.load().tlxmi_conv2d_splitk_supported(C.byref(d), s_) else 0


def bottleneck_seam_supported(K1, N1, N2, dtype):
    return bool(_lib.load().tlxmi_bottleneck_seam_supported(dt_code(dtype), int(K1), int(N1), int(N2)))


def bottleneck_seam_dec_supported(K1, N1, N2, rows, H, W, dtype):
    """Whether bottleneck_seam(..., y_stride2=True) has a kernel (tlxmi_bottleneck_seam_dec_supported: pure host code)."""
    return bool(_lib.load().tlxmi_bottleneck_seam_dec_supported(dt_code(dtype), int(K1), int(N1), int(N2), int(rows), int(H), int(W)))


def bottleneck_seam(t2, pk3, scale3, shift3, skip, pk1, scale1, shift1, proj=None, y_stride2=False):
    """One launch for the seam between two bottleneck blocks (tlxmi_bottleneck_seam): y = relu(conv3(t2) * scale3 + shift3 +
    skip); t1 = relu(conv1'(y) * scale1 + shift1).  t2 (N,H,W,K1), skip (N,H,W,N1) -> (y (N,H,W,N1), t1 (N,H,W,N2)).
    proj=(pk_d, scale_d, shift_d): `skip` is the block's INPUT (N,H,W,K1) and the projection shortcut conv_d + bn_d is computed
    inside the launch (tlxmi_bottleneck_seam_proj) instead of being read from a stored map.
    y_stride2: y is the compact map (N, (H+1)//2, (W+1)//2, N1) of the pixels with even h and w (tlxmi_bottleneck_seam_dec) — for a seam
    whose y is read by nothing but a 1x1 stride-2 convolution; t1 is the full map all the same."""
    need_gpu(t2, "input")
    N, H, W, ld = t2.shape
    if y_stride2 and proj is not None:
        raise RuntimeError("bottleneck_seam: no decimated form of the projection-shortcut seam")
    if skip.shape[:3] != t2.shape[:3] or skip.dtype != t2.dtype or not skip.is_contiguous() or not t2.is_contiguous():
        raise RuntimeError("bottleneck_seam: t2 / skip must be dense NHWC maps of one dtype and extent")
    y = torch.empty((N, (H + 1) // 2, (W + 1) // 2, pk3.Cout) if y_stride2 else (N, H, W, pk3.Cout), dtype=t2.dtype, device=t2.device)
    t1 = torch.empty((N, H, W, pk1.Cout), dtype=t2.dtype, device=t2.device)
    rows = N * H * W
    if _sizing():
        _note_act(t2.numel() * t2.element_size(), skip.numel() * skip.element_size(), y.numel() * y.element_size(), t1.numel() * t1.element_size())
    d = _lib.SeamDesc(dtype=dt_code(t2.dtype), rows=rows, K1=pk3.Cin, N1=pk3.Cout, N2=pk1.Cout, t2_ld=ld, skip_ld=skip.shape[-1],
                      y_ld=pk3.Cout, t1_ld=pk1.Cout, act=ACT_RELU)
    if y_stride2:
        name = "tlxmi_bottleneck_seam_dec"
        args = (C.byref(d), H, W, _p(t2), _p(pk3.buf), _p(scale3), _p(shift3), _p(skip), _p(y), _p(pk1.buf), _p(scale1), _p(shift1), _p(t1), _stream())
    elif proj is None:
        name = "tlxmi_bottleneck_seam"
        args = (C.byref(d), _p(t2), _p(pk3.buf), _p(scale3), _p(shift3), _p(skip), _p(y), _p(pk1.buf), _p(scale1), _p(shift1), _p(t1), _stream())
    else:
        name = "tlxmi_bottleneck_seam_proj"
        pkd, sd, hd = proj
        args = (C.byref(d), _p(t2), _p(pk3.buf), _p(scale3), _p(shift3), _p(skip), _p(pkd.buf), _p(sd), _p(hd), _p(y), _p(pk1.buf), _p(scale1),
                _p(shift1), _p(t1), _stream())
    skip_ch = pk3.Cout if proj is None else proj[0].Cin
    _timed(lambda: _lib.call(name, *args),
           lambda: ((rows * (pk3.Cin + skip_ch + pk1.Cout) + y.numel() + pk3.Cout * pk3.Cin + pk1.Cout * pk1.Cin) * t2.element_size(),
                    2 * rows * (pk3.Cout * pk3.Cin + pk1.Cout * pk1.Cin + (0 if proj is None else pk3.Cout * proj[0].Cin)),
                    (N, H, W, pk3.Cin, pk3.Cout, pk1.Cout, "seam+dec" if y_stride2 else "seam" if proj is None else "seam+proj", True)))
    return y, t1


def _proj_desc(t2, x2, pk, stride, out_ld, act, act_param, k2):
    N, Ho, Wo, ld = t2.shape
    k2 = x2.shape[-1] if k2 is None else int(k2)
    return _lib.ProjDesc(dtype=dt_code(t2.dtype), N=N, Ho=Ho, Wo=Wo, K1=pk.Cin - k2, K2=k2, Cout=pk.Cout, H2=x2.shape[1],
                         W2=x2.shape[2], stride=int(stride), x_ld=ld, x2_ld=x2.shape[-1], y_ld=out_ld, act=act, act_param=float(act_param),
                         flags=plan_flags())


def conv1x1_proj_supported(t2, x2, pk, stride, out=None, k2=None):
    """Whether conv1x1_proj takes these operands (tlxmi_conv1x1_proj_supported: pure host code)."""
    if (t2.dim() != 4 or x2.dim() != 4 or t2.dtype != pk.dtype or x2.dtype != pk.dtype or pk.R != 1 or pk.S != 1 or t2.shape[0] != x2.shape[0]
            or pk.Cin <= (x2.shape[-1] if k2 is None else k2) or not t2.is_contiguous() or not x2.is_contiguous() or t2.dtype not in (torch.float16, torch.float32)):
        return False
    N, Ho, Wo, _ = t2.shape
    # (the output is allocated by the call: any 16-byte aligned address apart from the inputs stands in for it here)
    d = _proj_desc(t2, x2, pk, stride, pk.Cout if out is None else out.shape[-1], ACT_NONE, 0.0, k2)
    y = C.c_void_p(16) if out is None else _p(out)
    return bool(_lib.load().tlxmi_conv1x1_proj_supported(C.byref(d), _p(t2), _p(x2), _p(pk.buf), y))


def conv1x1_proj_shapes_supported(t2_shape, x2_shape, pk, stride):
    """conv1x1_proj_supported for dense maps of these shapes and pk's dtype that do not exist yet (the same host predicate: three
    16-byte aligned addresses far apart stand in for the buffers, nothing is dereferenced)."""
    if len(t2_shape) != 4 or len(x2_shape) != 4 or pk.R != 1 or pk.S != 1 or t2_shape[0] != x2_shape[0] or pk.Cin <= x2_shape[-1] or pk.dtype not in (torch.float16, torch.float32):
        return False
    N, Ho, Wo, ld = t2_shape
    d = _lib.ProjDesc(dtype=dt_code(pk.dtype), N=N, Ho=Ho, Wo=Wo, K1=pk.Cin - x2_shape[-1], K2=x2_shape[-1], Cout=pk.Cout, H2=x2_shape[1],
                      W2=x2_shape[2], stride=int(stride), x_ld=ld, x2_ld=x2_shape[-1], y_ld=pk.Cout, act=ACT_NONE, act_param=0.0, flags=plan_flags())
    x, x2, y = (C.c_void_p(i << 40) for i in (1, 2, 3))
    return bool(_lib.load().tlxmi_conv1x1_proj_supported(C.byref(d), x, x2, _p(pk.buf), y))


def conv1x1_proj(t2, x2, pk, stride, shift=None, act=ACT_NONE, act_param=0.0, out=None, k2=None):
    """y = act([t2 | x2 at `stride`] . W'^T + shift) in one launch (tlxmi_conv1x1_proj): the expand conv of a ResNet transition block
    with its 1x1 projection shortcut as extra K.  t2 (N,Ho,Wo,>=K1), x2 (N,H2,W2,>=K2) dense NHWC fp16 maps (their last extent is the
    pitch; k2: the channels of x2 that are read, default all; K1 = pk.Cin - K2), pk = PackedFilter of [Cout][K1 + K2] with both BatchNorm scales folded in -> y (N,Ho,Wo,Cout), or `out` (a wider map)."""
    need_gpu(t2, "input")
    need_gpu(x2, "shortcut input")
    if t2.dim() != 4 or x2.dim() != 4 or not t2.is_contiguous() or not x2.is_contiguous() or t2.shape[0] != x2.shape[0]:
        raise RuntimeError("conv1x1_proj: t2 / x2 must be dense NHWC maps of one batch")
    if t2.dtype != pk.dtype or x2.dtype != pk.dtype:
        raise RuntimeError(f"conv1x1_proj: input dtypes {t2.dtype} / {x2.dtype} != packed filter dtype {pk.dtype}")
    N, Ho, Wo, _ = t2.shape
    if out is None:
        out = torch.empty((N, Ho, Wo, pk.Cout), dtype=t2.dtype, device=t2.device)
    d = _proj_desc(t2, x2, pk, stride, out.shape[-1], act, act_param, k2)
    M = N * Ho * Wo
    es = t2.element_size()
    if _sizing():
        _note_act(t2.numel() * es, x2.numel() * es, M * d.y_ld * es)
    args = (C.byref(d), _p(t2), _p(x2), _p(pk.buf), _p(shift), _p(out), _stream())
    # algorithmic bytes: the rows of t2, the pixels of x2 the stride selects, the output, the filter
    _timed(lambda: _lib.call("tlxmi_conv1x1_proj", *args),
           lambda: ((M * (d.K1 + d.K2) + M * pk.Cout + pk.Cout * pk.Cin) * es, 2 * M * pk.Cout * pk.Cin,
                    (N, Ho, Wo, d.K1, pk.Cout, d.K2, "expand+proj", int(stride))))
    return out


def group_conv2d(x, pk, stride=1, padding=0, dilation=1, scale=None, shift=None, res=None, act=ACT_NONE,
                 act_param=0.0, res_after_act=False):
    """Grouped convolution (+ folded BatchNorm / bias, activation, residual): x (N,H,W,Cin) NHWC with exactly the
    filter's input channels -> (N,Ho,Wo,Cout).  pk: PackedGroupFilter."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    if x.dtype != pk.dtype:
        raise RuntimeError(f"group_conv2d: input dtype {x.dtype} != packed filter dtype {pk.dtype}")
    if ld != pk.Cin:
        raise RuntimeError(f"group_conv2d: input has {ld} channels, filter expects {pk.Cin}")
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dh, dw = _pair(dilation)
    Ho = (H + 2 * ph - dh * (pk.R - 1) - 1) // sh + 1
    Wo = (W + 2 * pw - dw * (pk.S - 1) - 1) // sw + 1
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError(f"group_conv2d: empty output {Ho}x{Wo} for input {H}x{W}")
    out = torch.empty((N, Ho, Wo, pk.Cout), dtype=x.dtype, device=x.device)
    if res is not None and res.dtype != x.dtype:
        raise RuntimeError("group_conv2d: residual dtype mismatch")
    d = _lib.ConvDesc(dtype=dt_code(x.dtype), N=N, H=H, W=W, C=pk.Cin, Cout=pk.Cout, R=pk.R, S=pk.S,
                      stride_h=sh, stride_w=sw, pad_h=ph, pad_w=pw, dil_h=dh, dil_w=dw, Ho=Ho, Wo=Wo,
                      x_ld=ld, y_ld=pk.Cout, res_ld=(res.shape[-1] if res is not None else 0),
                      y_nstride=0, res_nstride=0, act=act, act_param=float(act_param),
                      flags=(EPI_RES_AFTER_ACT if res_after_act else 0) | plan_flags())
    args = (C.byref(d), pk.groups, _p(x), _p(pk.buf), _p(scale), _p(shift), _p(res), _p(out), _stream())
    if _sizing():
        _note_act(x.numel() * x.element_size(), out.numel() * out.element_size(), res.numel() * res.element_size() if res is not None else 0)
    M = N * Ho * Wo
    cg = pk.Cin // pk.groups
    _timed(lambda: _lib.call("tlxmi_group_conv2d", *args),
           lambda: ((N * H * W * pk.Cin + M * pk.Cout * (2 if res is not None else 1) + pk.Cout * cg * pk.R * pk.S) * x.element_size(),
                    2 * M * pk.Cout * cg * pk.R * pk.S, (N, H, W, pk.Cin, pk.Cout, pk.R, sh, f"g{pk.groups}")))
    return out


def linear(x, pk, bias=None, res=None, act=ACT_NONE, out=None):
    """x (..., K) -> (..., Cout): the H=W=1 case of the implicit GEMM, bias as epilogue shift."""
    need_gpu(x, "input")
    shp = x.shape
    if not x.is_contiguous():
        x = x.contiguous()
    rows = x.numel() // shp[-1]
    x4 = x.view(rows, 1, 1, shp[-1])
    r4 = None
    if res is not None:
        if not res.is_contiguous():
            res = res.contiguous()
        r4 = res.view(rows, 1, 1, pk.Cout)
    o4 = None
    if out is not None:
        o4 = out.view(rows, 1, 1, pk.Cout)
    if x.dtype != pk.dtype:
        raise RuntimeError(f"linear: input dtype {x.dtype} != packed filter dtype {pk.dtype}")
    tail = _linear_tail(rows, shp[-1], pk, x) if (_probe is None and pk.R == 1 and pk.S == 1) else None
    if tail is not None:
        # Whole rounds of 256 x 256 tiles on the persistent kernel, the rows of the short last round as K slices side by side +
        # the deterministic slice-order reduction (bias, residual, activation there): the balanced tail WITHOUT giving up the
        # tile's arithmetic intensity (a K slice of a tile reads as many operand bytes per FLOP as the whole tile)
        m_lo, slices = tail
        y = out.view(rows, pk.Cout) if out is not None else torch.empty((rows, pk.Cout), dtype=x.dtype, device=x.device)
        x2 = x.view(rows, shp[-1])
        r2 = res.view(rows, pk.Cout) if res is not None else None
        conv2d(x2[:m_lo].view(m_lo, 1, 1, shp[-1]), pk, shift=bias, res=(r2[:m_lo].view(m_lo, 1, 1, pk.Cout) if r2 is not None else None),
               act=act, out=y[:m_lo].view(m_lo, 1, 1, pk.Cout))
        hi = rows - m_lo
        part = torch.empty((slices, hi, pk.Cout), dtype=torch.float32, device=x.device)      # fp32 partial sums
        _lib.call("tlxmi_linear_splitk", dt_code(x.dtype), hi, shp[-1], pk.Cout, shp[-1], _p(x2[m_lo:]), _p(pk.buf), slices, _p(part),
                  None, _p(bias), _p(r2[m_lo:] if r2 is not None else None), pk.Cout if r2 is not None else 0, act, C.c_float(0.0), 0,
                  _p(y[m_lo:]), pk.Cout, _stream())
        return y.view(*shp[:-1], pk.Cout)
    splits = _linear_splits(rows, shp[-1], pk, x) if (out is None and _probe is None and pk.R == 1 and pk.S == 1) else 0
    if splits:
        # few rows, large filter (classifier heads): K slices side by side + a deterministic reduction (tlxmi_linear_splitk)
        part = torch.empty((splits, rows, pk.Cout), dtype=torch.float32, device=x.device)      # fp32 partial sums
        y = torch.empty((rows, pk.Cout), dtype=x.dtype, device=x.device)
        _lib.call("tlxmi_linear_splitk", dt_code(x.dtype), rows, shp[-1], pk.Cout, shp[-1], _p(x), _p(pk.buf), splits, _p(part),
                  None, _p(bias), _p(res), pk.Cout if res is not None else 0, act, C.c_float(0.0), 0, _p(y), pk.Cout, _stream())
        return y.view(*shp[:-1], pk.Cout)
    y = conv2d(x4, pk, shift=bias, res=r4, act=act, out=o4)
    return y.view(*shp[:-1], pk.Cout)


def _linear_tail(rows, K, pk, x):
    """(rows of the whole rounds, K slices of the rest) for a Linear whose 256 x 256 tiles are r whole rounds on the CUs this
    launch is planned for plus a last round at most half full — ViT-B/16 proj / fc2 at batch 256: 2.32 rounds paid as 3, and
    batch 222 runs 6 % fewer images per second than batch 220 (tools/batch_quant.py) — else None.  The persistent kernel then
    runs exactly r rounds and the leftover rows go to tlxmi_linear_splitk.  OFF by default (set_option("tail_splitk", True) for the
    A/B): measured slower than the idle round it removes (the option table above); the in-kernel half-height tiles of
    gemm_stream.hip are what the product runs."""
    if not _options["tail_splitk"] or pk.Cin != K or pk.Cin_pad != K or pk.Cout < 256:
        return None
    es = x.element_size()
    kt = K * es // 128                      # K tiles of 128 bytes
    if (K * es) % 128 or kt < _TAIL_MIN_KTILES or (pk.Cout * es) % 16:
        return None
    idx = x.device.index if x.device.index is not None else torch.cuda.current_device()
    if idx not in _cus:
        _cus[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    cus = _cus[idx] // 2 if (plan_flags() & _lib.PLAN_SHARED_HALF) else _cus[idx]
    grid = max(8, cus & ~7)
    nt = (pk.Cout + 255) // 256
    tiles = ((rows + 255) // 256) * nt
    r, rem = divmod(tiles, grid)
    if r < 1 or rem == 0 or 2 * rem > grid:
        return None
    m_lo = (r * grid // nt) * 256
    hi = rows - m_lo
    if m_lo <= 0 or hi <= 0:
        return None
    t128 = ((hi + 127) // 128) * ((pk.Cout + 127) // 128)
    best = 0
    for s_ in range(2, 9):
        if kt % s_ or kt // s_ < 4:
            continue
        best = s_
        if t128 * s_ >= 2 * grid:
            break
    if not best or hi * pk.Cout * 4 * best >= (1 << 31):
        return None
    return m_lo, best


_TAIL_MIN_KTILES = 12      # (K >= 768 in fp16)


def _linear_splits(rows, K, pk, x):
    """Number of K slices for a Linear with few rows (0: run it as one GEMM).  set_option("splitk", False) turns the path off (A/B)."""
    if not _options["splitk"] or rows > 512 or pk.Cin != K or pk.Cin_pad != K:
        return 0
    es = x.element_size()
    if K * es < 4096 or pk.Cout * K * es < 3000000 or (pk.Cout * es) % 16:      # a filter of >= 3 MB with K >= 2048 (fp16): VGG / AlexNet
        # heads (round 2) and, round 4, ResNet's 2048 -> 1000 head (32 tiles of 64 x 64 per half batch, each walking all of K: 3.403 ->
        # 3.387 ms per ResNet-50 forward, tools/ab_tmp.py)
        return 0
    idx = x.device.index if x.device.index is not None else torch.cuda.current_device()
    if idx not in _cus:
        _cus[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    tiles = ((rows + 63) // 64) * ((pk.Cout + 63) // 64)
    kt = K * es // 128                      # K tiles of 128 bytes
    best = 0
    for s_ in range(2, 65):
        if kt % s_ or kt // s_ < 4:         # at least 4 K tiles per slice: the partial sums stay a small share of the traffic
            continue
        best = s_
        if tiles * s_ >= 3 * _cus[idx]:
            break
    if best and rows * pk.Cout * es * best >= (1 << 31):
        return 0
    return best


def mlp_seam_supported(rows, K, hidden, N, dtype):
    """Whether mlp_seam() takes these rows: tlxmi_mlp_seam_supported answers for the shape only, the rows of x (K channels) and of
    res / out (N channels) must each stay under the 2 GiB the 32-bit buffer offsets address (the call refuses them otherwise)."""
    return bool(_options["mlp_seam"] and dtype == torch.float16 and rows >= 4096 and rows * max(K, N) * 2 < (1 << 31)
                and _lib.load().tlxmi_mlp_seam_supported(F16, int(K), int(hidden), int(N)))


def mlp_seam(x, pk1, b1, pk2, b2, res, out=None):
    """out = fc2(gelu(fc1(x) + b1)) + b2 + res in ONE launch (tlxmi_mlp_seam): x (..., K) fp16, pk1 / pk2 the packed fc1 / fc2 filters, res
    (..., N) the residual rows; out may be res (in place: a row is read before it is written by the lane that owns it)."""
    need_gpu(x, "input")
    shp = x.shape
    x = x if x.is_contiguous() else x.contiguous()
    K = shp[-1]
    rows = x.numel() // K
    N = pk2.Cout
    if not res.is_contiguous():
        raise RuntimeError("mlp_seam: the residual must be dense")
    y = out if out is not None else torch.empty((*shp[:-1], N), dtype=x.dtype, device=x.device)
    if _sizing():
        _note_act(rows * max(K, N) * x.element_size())
    _timed(lambda: _lib.call("tlxmi_mlp_seam", dt_code(x.dtype), rows, K, pk1.Cout, N, _p(x), K, _p(pk1.buf), _p(b1), _p(pk2.buf), _p(b2), _p(res), N,
                             _p(y), N, _stream()),
           lambda: ((rows * (K + 2 * N) + 2 * pk1.Cout * K) * 2, 2 * rows * pk1.Cout * (K + N), (rows, 1, 1, K, N, pk1.Cout, "mlp seam", True)))
    return y


def linear_ln_supported(rows, K, Cout, dtype, act=ACT_NONE, with_res=False, producer=False):
    """Whether a Linear of this shape takes the folded-LayerNorm path (tlxmi_linear_stats with_res / tlxmi_linear_ln): fp16 on the
    persistent 256 x 256 GEMM kernel, rows enough to fill it (below ~2 k rows the tiled kernels of the dispatcher win)."""
    # tools/batch_table.py (round 5): inside a two-stream forward the other half's launches fill what a persistent GEMM with few tiles
    # leaves idle, so the fold pays from ~2 k rows (ViT-B/16 batch 64 = 2 x 32 images: +9 %); a forward on ONE stream at that size is
    # faster on the dispatcher's smaller tiles + LayerNorm launches (ViT-B/16 batch 32: -6 %, Swin-B batch 32: -7 %, batch 64: equal)
    min_rows = _options["lnfold_min_rows"] if in_halves() else max(_options["lnfold_min_rows"], _options["lnfold_min_rows_one_stream"])
    if not _options["lnfold"] or dtype != torch.float16 or rows < min_rows:
        return False
    return bool(_lib.load().tlxmi_linear_ln_supported(F16, int(rows), int(K), int(Cout), int(act), 1 if with_res else 2 if producer else 0))


class LinearLN:
    """A Linear with the LayerNorm in front of it folded in (include/tlxmi.h, tlxmi_linear_ln): packed W * gamma, c1 = row sums of the
    values as packed, c2 = bias + W @ beta."""

    def __init__(self, w_out_in, bias, gamma, beta, dtype):
        w = w_out_in.detach().float()
        g, b = gamma.detach().float().to(w.device), beta.detach().float().to(w.device)
        wg = w * g[None, :]
        self.pk = PackedFilter(wg.view(w.shape[0], w.shape[1], 1, 1).contiguous(), dtype)
        self.c1 = wg.to(dtype).double().sum(dim=1).float().contiguous()
        self.c2 = (w.double() @ b.double() + (bias.detach().double().to(w.device) if bias is not None else 0.0)).float().contiguous()
        self.K, self.Cout = w.shape[1], w.shape[0]


def linear_stats(x, pk, bias=None, res=None, out=None):
    """y = x W^T + bias (+ res) as linear(), plus per row (sum, sum of squares) of y over every 256-channel tile column from the same
    epilogue: returns (y, partials (rows, 4, 2) fp32, pair p < ceil(Cout / 256) written) — the statistics of the LayerNorm that follows,
    without a pass over y; linear_ln takes them as they are."""
    need_gpu(x, "input")
    shp = x.shape
    if not x.is_contiguous():
        x = x.contiguous()
    K = shp[-1]
    rows = x.numel() // K
    if x.dtype != pk.dtype:
        raise RuntimeError(f"linear_stats: input dtype {x.dtype} != packed filter dtype {pk.dtype}")
    if res is not None and (not res.is_contiguous() or res.dtype != x.dtype):
        raise RuntimeError("linear_stats: the residual must be a dense tensor of the input's dtype")
    y = out if out is not None else torch.empty((*shp[:-1], pk.Cout), dtype=x.dtype, device=x.device)
    part = torch.empty((rows, 4, 2), dtype=torch.float32, device=x.device)      # pair p < ceil(Cout / 256) written
    if _sizing():
        _note_act(rows * max(K, pk.Cout) * x.element_size())
    _timed(lambda: _lib.call("tlxmi_linear_stats", dt_code(x.dtype), rows, K, pk.Cout, K, pk.Cout, _p(x), _p(pk.buf), _p(bias), _p(res),
                             pk.Cout if res is not None else 0, _p(y), _p(part), plan_flags(), _stream()),
           lambda: ((rows * K + rows * pk.Cout * (2 if res is not None else 1) + pk.Cout * K) * x.element_size() + part.numel() * 4,
                    2 * rows * pk.Cout * K, (rows, 1, 1, K, pk.Cout, 1, 1, res is not None)))
    return y, part


def linear_ln(x, prep, part, eps, act=ACT_NONE, out=None):
    """act(Linear(LayerNorm(x))) on the RAW rows x (..., K): `part` = the (rows, 4, 2) pairs of (sum, sum of squares) the linear_stats
    launch that wrote x left (the first ceil(K / 256) of a row are read); mean / rstd of a row are formed inside the GEMM and applied in its epilogue."""
    need_gpu(x, "input")
    shp = x.shape
    if not x.is_contiguous():
        x = x.contiguous()
    rows = x.numel() // shp[-1]
    if tuple(part.shape) != (rows, 4, 2) or part.dtype != torch.float32 or not part.is_contiguous():
        raise RuntimeError(f"linear_ln: statistics of shape {tuple(part.shape)} for {rows} rows (expected {(rows, 4, 2)} fp32)")
    y = out if out is not None else torch.empty((*shp[:-1], prep.Cout), dtype=x.dtype, device=x.device)
    if _sizing():
        _note_act(rows * max(prep.K, prep.Cout) * x.element_size())
    _timed(lambda: _lib.call("tlxmi_linear_ln", dt_code(x.dtype), rows, prep.K, prep.Cout, prep.K, prep.Cout, _p(x), _p(prep.pk.buf), _p(prep.c1),
                             _p(prep.c2), _p(part), C.c_float(float(eps)), act, _p(y), plan_flags(), _stream()),
           lambda: ((rows * prep.K + rows * prep.Cout + prep.Cout * prep.K) * x.element_size() + part.numel() * 4,
                    2 * rows * prep.Cout * prep.K, (rows, 1, 1, prep.K, prep.Cout, 1, 1, False)))
    return y


def dwconv2d(x, w_rsc, stride=1, padding=0, dilation=1, scale=None, shift=None, act=ACT_NONE, act_param=0.0, out_hw=None,
             x_ld=None, out=None, out_ld=None):
    """x_ld: the pixel pitch when x is a 16-byte aligned column slice of a wider map (a view: the filter's channels are read);
    out / out_ld: write into a 16-byte aligned column slice of a wider buffer (pixel pitch out_ld, default out's last axis)."""
    need_gpu(x, "input")
    N, H, W, Cc = x.shape
    R, S, Cw = w_rsc.shape
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dh, dw = _pair(dilation)
    Ho = (H + 2 * ph - dh * (R - 1) - 1) // sh + 1
    Wo = (W + 2 * pw - dw * (S - 1) - 1) // sw + 1
    if out_hw is not None:      # one-sided end padding ('SAME' at stride 2): the last windows read zeros past the edge
        Ho, Wo = int(out_hw[0]), int(out_hw[1])
    y = out if out is not None else torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    y_ld = Cc if out is None else int(out_ld if out_ld is not None else out.shape[-1])
    d = _lib.DwConvDesc(dtype=dt_code(x.dtype), N=N, H=H, W=W, C=Cw, R=R, S=S, stride_h=sh, stride_w=sw, pad_h=ph,
                        pad_w=pw, dil_h=dh, dil_w=dw, Ho=Ho, Wo=Wo, x_ld=Cc if x_ld is None else int(x_ld), y_ld=y_ld, act=act,
                        act_param=float(act_param))
    _lib.call("tlxmi_dwconv2d", C.byref(d), _p(x), _p(w_rsc), _p(scale), _p(shift), _p(y), _stream())
    return y


def _dwconv7_desc(x, Cc, y_ld):
    N, H, W, ld = x.shape
    return _lib.DwConv7Desc(dtype=dt_code(x.dtype), N=N, H=H, W=W, C=Cc, R=7, S=7, stride_h=1, stride_w=1, pad_h=3, pad_w=3, dil_h=1, dil_w=1,
                            x_ld=ld, y_ld=y_ld)


def dwconv7_supported(x, Cc=None):
    """Whether dwconv7_stats() runs tlxmi_dwconv7_stats on this dense NHWC map (the "dwconv7" option on, fp16, the library takes the shape)."""
    Cc = x.shape[-1] if Cc is None else Cc
    return bool(_options["dwconv7"] and x.dtype == torch.float16 and x.is_contiguous()
                and _lib.load().tlxmi_dwconv7_stats_supported(C.byref(_dwconv7_desc(x, Cc, Cc))))


def dwconv7_stats(x, w_rsc, bias=None, stats=True, fused=None):
    """ConvNeXt's depthwise conv (convnext.py:91-93: 7x7, stride 1, padding 3, + bias): x (N, H, W, C) NHWC, w_rsc [7][7][C], bias fp32 [C]
    or None -> (y (N, H, W, C), part).  On tlxmi_dwconv7_stats (fp16, the "dwconv7" option, shapes the library takes) part is the
    (N*H*W, 4, 2) fp32 (sum, sum of squares) per 256-channel plane of the fp32 y before rounding — what linear_ln() reads — when
    `stats`, else None.  Otherwise tlxmi_dwconv2d runs and part is None: the caller keeps its layernorm() launch.
    fused=True / False forces one form (tests, tools/)."""
    need_gpu(x, "input")
    N, H, W, Cc = x.shape
    if tuple(w_rsc.shape) != (7, 7, Cc) or w_rsc.dtype != x.dtype or not x.is_contiguous():
        raise RuntimeError(f"dwconv7_stats: a dense NHWC map and a [7][7][{Cc}] filter of its dtype are expected, got {tuple(x.shape)} / {tuple(w_rsc.shape)}")
    if fused is None:
        fused = dwconv7_supported(x)
    es = x.element_size()
    if _sizing():
        _note_act(x.numel() * es)
    y = torch.empty_like(x) if fused else None
    part = torch.empty((N * H * W, 4, 2), dtype=torch.float32, device=x.device) if fused and stats else None      # pair p < ceil(C / 256) written

    def launch():
        if not fused:
            return dwconv2d(x, w_rsc, 1, 3, 1, None, bias)
        _lib.call("tlxmi_dwconv7_stats", C.byref(_dwconv7_desc(x, Cc, Cc)), _p(x), _p(w_rsc), _p(bias), _p(y), _p(part), _stream())
        return y
    y = _timed(launch, lambda: (2 * x.numel() * es + 49 * Cc * es + (part.numel() * 4 if part is not None else 0), 2 * 49 * x.numel(),
                                (N, H, W, Cc, Cc, 7, 1, "dwconv7" if fused else "dwconv2d")))
    return y, part


_conv2d = conv2d        # the unfused arm of sepconv2d (a tool that wraps E.conv2d sees the pair as one separable conv)


def sepconv2d(x, w_dw, dw_scale, dw_shift, pk, pw_scale, pw_shift, dilation, act=ACT_RELU, act_param=0.0, out=None, out_ld=None,
              fused=None):
    """SeparableConvBNReLU (layer_libs.py:98-133): depthwise 3x3 (stride 1, padding = dilation) + folded BN, rounded to the
    activation dtype, then pointwise 1x1 + folded BN + act.  x (N, H, W, ld) NHWC with C = w_dw.shape[2] channels used;
    w_dw [3][3][C]; pk: PackedFilter of the [Cout][C] pointwise filter -> y (N, H, W, Cout), or written into `out` (a column slice
    of a wider buffer, pixel pitch out_ld).  One launch (tlxmi_sepconv2d) when the "sepconv" option is on, the precision is
    fp16, the conv is dilated and the library takes the shape; otherwise tlxmi_dwconv2d then tlxmi_conv2d (fp32 always: the
    parity reference).  Dilation 1 keeps the pair: there the depthwise runs on dwconv_strip_kernel, and the pair measured faster
    than the fused kernel at DeepLabV3+'s decoder shapes.  fused=True / False forces one form (tests, tools/)."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    R, S, Cc = w_dw.shape
    d = int(dilation)
    if (R, S) != (3, 3) or pk.R != 1 or pk.S != 1 or pk.Cin != Cc:
        raise RuntimeError(f"sepconv2d: depthwise {R}x{S}x{Cc} -> pointwise {pk.Cout}x{pk.Cin}x{pk.R}x{pk.S} is not a separable 3x3 conv")
    if x.dtype != pk.dtype or w_dw.dtype != x.dtype or ld < Cc or not x.is_contiguous():
        raise RuntimeError("sepconv2d: x must be a dense NHWC map of the filters' dtype with at least C channels")
    if out is None:
        out = torch.empty((N, H, W, pk.Cout), dtype=x.dtype, device=x.device)
        out_ld = pk.Cout
    elif out_ld is None:
        out_ld = out.shape[-1]
    es = x.element_size()
    M = N * H * W
    if _sizing():
        _note_act(x.numel() * es, M * Cc * es, M * out_ld * es)
    desc = _lib.SepConvDesc(dtype=dt_code(x.dtype), N=N, H=H, W=W, C=Cc, Cout=pk.Cout, R=3, S=3, stride_h=1, stride_w=1, pad_h=d,
                            pad_w=d, dil_h=d, dil_w=d, x_ld=ld, y_ld=out_ld, act=act, act_param=float(act_param))
    if fused is None:
        fused = bool(_options["sepconv"] and x.dtype == torch.float16 and d > 1 and _lib.load().tlxmi_sepconv2d_supported(C.byref(desc)))

    def launch():
        if fused:
            _lib.call("tlxmi_sepconv2d", C.byref(desc), _p(x), _p(w_dw), _p(dw_scale), _p(dw_shift), _p(pk.buf), _p(pw_scale),
                      _p(pw_shift), _p(out), _stream())
        else:
            t = dwconv2d(x, w_dw, 1, d, d, dw_scale, dw_shift)
            _conv2d(t, pk, 1, 0, 1, pw_scale, pw_shift, act=act, act_param=act_param, out=out, out_ld=out_ld)
    _timed(launch, lambda: ((M * Cc + M * pk.Cout + 9 * Cc + pk.Cout * Cc) * es, 2 * M * Cc * 9 + 2 * M * pk.Cout * Cc,
                            (N, H, W, Cc, pk.Cout, "sep", d, fused)))      # the pair is one entry
    return out


def preact_conv1x1(x, pre_scale, pre_shift, pk, scale=None, shift=None, act=ACT_NONE, out=None, out_ld=None, fused=None, pre_act=ACT_RELU):
    """BNACConvLayer with a 1x1 filter (densenet.py:31-46): y = act(conv1x1(pre_act(x * pre_scale + pre_shift)) * scale + shift).
    x (N, H, W, x_ld) NHWC (or (rows, x_ld)): the first K = pk.Cin channels of each pixel are the operand — a channel prefix of a dense
    block's buffer; the columns behind K are never used, whatever they hold.  pre_scale / pre_shift: fp32 [K] -> y (N, H, W, Cout), or
    written into `out` (a column slice of a wider buffer, pixel pitch out_ld).  One launch (tlxmi_preact_conv1x1) when the "preact"
    option is on, the precision is fp16 and the library takes the shape; otherwise tlxmi_affine_act into a dense K-channel temporary
    then tlxmi_conv2d (fp32 always: the parity reference).  fused=True / False forces one form (tests, tools/)."""
    need_gpu(x, "input")
    if x.dim() == 2:
        x = x.view(x.shape[0], 1, 1, x.shape[1])
    N, H, W, ld = x.shape
    K = pk.Cin
    if pk.R != 1 or pk.S != 1 or x.dtype != pk.dtype or ld < K or not x.is_contiguous() or K % vec(x.dtype):
        raise RuntimeError(f"preact_conv1x1: x must be a dense NHWC map of the filter's dtype with at least K = {K} channels (a multiple of "
                           f"{vec(x.dtype)}) and the filter 1x1; got {tuple(x.shape)} {x.dtype} for a {pk.R}x{pk.S} filter")
    if pre_scale is None or pre_shift is None or pre_scale.numel() != K or pre_shift.numel() != K:
        raise RuntimeError(f"preact_conv1x1: pre_scale / pre_shift must hold K = {K} values")
    if out is None:
        out = torch.empty((N, H, W, pk.Cout), dtype=x.dtype, device=x.device)
        out_ld = pk.Cout
    elif out_ld is None:
        out_ld = out.shape[-1]
    es = x.element_size()
    M = N * H * W
    if _sizing():
        _note_act(x.numel() * es, M * out_ld * es)
    if fused is None:
        fused = bool(_options["preact"] and x.dtype == torch.float16
                     and _lib.load().tlxmi_preact_conv1x1_supported(F16, M, K, pk.Cout, ld, out_ld, pre_act, act))
    if not fused:
        t = torch.empty((N, H, W, K), dtype=x.dtype, device=x.device)
        _lib.call("tlxmi_affine_act", _p(x), _p(pre_scale), _p(pre_shift), None, _p(t), dt_code(x.dtype), M, K, ld, 0, K, pre_act, 0.0, 0,
                  _stream())
        conv2d(t, pk, 1, 0, 1, scale, shift, act=act, out=out, out_ld=out_ld)
        return out
    args = (F16, M, K, pk.Cout, ld, out_ld, _p(x), _p(pre_scale), _p(pre_shift), pre_act, _p(pk.buf), _p(scale), _p(shift), act, _p(out), _stream())
    _timed(lambda: _lib.call("tlxmi_preact_conv1x1", *args),
           lambda: ((M * K + M * pk.Cout + pk.Cout * K) * es, 2 * M * pk.Cout * K, (N, H, W, K, pk.Cout, "preact")))
    return out


def mul(a, b, cols=None, out=None):
    """Elementwise product (VAN's gate `x * attn`, van.py:100) on tlxmi_mul: a, b dense tensors of one dtype whose rows are their last
    axis — the first `cols` columns of each row are multiplied (default: all of a's), so a and b may be pitched differently -> y with
    `cols` columns, or written into `out` (any pitch >= cols)."""
    need_gpu(a, "input")
    need_gpu(b, "input")
    Cc = a.shape[-1] if cols is None else int(cols)
    rows = a.numel() // a.shape[-1]
    if a.dtype != b.dtype or not a.is_contiguous() or not b.is_contiguous() or b.numel() // b.shape[-1] != rows or a.shape[-1] < Cc or b.shape[-1] < Cc:
        raise RuntimeError(f"mul: two dense tensors of one dtype with the same rows and at least {Cc} columns are expected, got {tuple(a.shape)} {a.dtype} / {tuple(b.shape)} {b.dtype}")
    if out is None:
        out = torch.empty(tuple(a.shape[:-1]) + (Cc,), dtype=a.dtype, device=a.device)
    elif out.dtype != a.dtype or not out.is_contiguous() or out.shape[-1] < Cc or out.numel() // out.shape[-1] != rows:
        raise RuntimeError("mul: out must be a dense tensor of the operands' dtype and rows")
    _lib.call("tlxmi_mul", _p(a), _p(b), _p(out), dt_code(a.dtype), rows, Cc, a.shape[-1], b.shape[-1], out.shape[-1], _stream())
    return out


def _lka_dw_desc(t, Cc, y_ld):
    N, H, W, ld = t.shape
    return _lib.LkaDwDesc(dtype=dt_code(t.dtype), N=N, H=H, W=W, C=Cc, x_ld=ld, y_ld=y_ld)


# Shapes the fused kernels keep by default: those that measured faster than the old arm on one MI355X at batch 256 and 128 (tools/van_bench.py,
# profiles/van/van_bench_b256.txt).  tlxmi_lka_dw won on planes of 56 x 56, 28 x 28 and 14 x 14 (0.66 - 0.94 of the two launches) and lost on
# 7 x 7 (1.8 - 2.8 x: 49 of a workgroup's 128 pixel slots have work); nothing between 49 and 196 pixels was measured, so the smallest measured win
# is the threshold.  tlxmi_lka_gate won at C = 32 and 64 (0.39 - 0.79 of the four launches), tied at 160 (1.04 at batch 256, 0.84 at 128) and lost
# at 256 (2.2 - 2.8 x: every wave re-reads 256 KiB of filters); 96 and 128 were not measured, so 64 is the limit.
LKA_DW_MIN_PIXELS = 196
LKA_GATE_MAX_C = 64


def lka_dw_supported(t, Cc=None):
    """Whether lka_dw() runs tlxmi_lka_dw on this NHWC map by default: the "lka" option on, fp16, the library takes the shape, and the plane
    has at least LKA_DW_MIN_PIXELS pixels (smaller planes measured slower than two tlxmi_dwconv2d launches)."""
    Cc = t.shape[-1] if Cc is None else Cc
    return bool(_options["lka"] and t.dtype == torch.float16 and t.is_contiguous() and t.shape[1] * t.shape[2] >= LKA_DW_MIN_PIXELS
                and _lib.load().tlxmi_lka_dw_supported(C.byref(_lka_dw_desc(t, Cc, Cc))))


def lka_dw(t, w0, b0, w1, b1, fused=None):
    """LKA.conv0 -> LKA.conv_spatial (van.py:87-98): depthwise 5x5 (padding 2) then depthwise 7x7 at dilation 3 (padding 9), each + bias, the
    map between them rounded to the activation dtype.  t (N, H, W, ld) NHWC with the first C = w0.shape[2] channels used; w0 [5][5][C],
    w1 [7][7][C]; b0, b1 fp32 [C] or None -> y (N, H, W, C).  One launch (tlxmi_lka_dw, the map between the convs kept in LDS) when the
    "lka" option is on, the precision is fp16, the library takes the shape and the plane has at least LKA_DW_MIN_PIXELS pixels; otherwise
    two tlxmi_dwconv2d launches (fp32 always: the parity reference).  fused=True / False forces one form (tests, tools/)."""
    need_gpu(t, "input")
    N, H, W, ld = t.shape
    Cc = w0.shape[2]
    if tuple(w0.shape) != (5, 5, Cc) or tuple(w1.shape) != (7, 7, Cc) or w0.dtype != t.dtype or w1.dtype != t.dtype or ld < Cc or not t.is_contiguous():
        raise RuntimeError(f"lka_dw: a dense NHWC map with at least C channels and [5][5][C] / [7][7][C] filters of its dtype are expected, got "
                           f"{tuple(t.shape)} {t.dtype} / {tuple(w0.shape)} / {tuple(w1.shape)}")
    if fused is None:
        fused = lka_dw_supported(t, Cc)
    es = t.element_size()
    if _sizing():
        _note_act(t.numel() * es)
    M = N * H * W

    def launch():
        if fused:
            y = torch.empty((N, H, W, Cc), dtype=t.dtype, device=t.device)
            _lib.call("tlxmi_lka_dw", C.byref(_lka_dw_desc(t, Cc, Cc)), _p(t), _p(w0), _p(b0), _p(w1), _p(b1), _p(y), _stream())
            return y
        y = dwconv2d(dwconv2d(t, w0, 1, 2, 1, None, b0), w1, 1, 9, 3, None, b1)
        return y if ld == Cc else y[..., :Cc].contiguous()
    return _timed(launch, lambda: ((2 * M * Cc + 74 * Cc) * es, 2 * 74 * M * Cc, (N, H, W, Cc, Cc, "lka_dw" if fused else "dwconv2d x2")))


def _lka_gate_desc(rows, Cc, dtype):
    return _lib.LkaGateDesc(dtype=dt_code(dtype), rows=rows, C=Cc, a1_ld=Cc, t_ld=Cc, res_ld=Cc, y_ld=Cc)


def lka_gate_supported(rows, Cc, dtype):
    """Whether lka_gate() runs tlxmi_lka_gate on dense (rows, C) operands by default: the "lka" option on, fp16, the library takes the shape,
    and C <= LKA_GATE_MAX_C (wider stages measured no faster than the four launches)."""
    return bool(_options["lka"] and dtype == torch.float16 and Cc <= LKA_GATE_MAX_C
                and _lib.load().tlxmi_lka_gate_supported(C.byref(_lka_gate_desc(rows, Cc, dtype))))


def lka_gate(a1, t, pk1, scale1, shift1, pk2, scale2, shift2, res, res_scale, fused=None):
    """LKA.conv1 -> the gate -> Attention.proj_2 -> layer scale and shortcut (van.py:99-100, :119-120, :146):
        a2 = conv1x1(a1; pk1) * scale1 + shift1;   g = t * a2 (rounded to the activation dtype);
        y  = res * res_scale + conv1x1(g; pk2) * scale2 + shift2
    a1, t, res: dense (N, H, W, C) or (rows, C) of one dtype; pk1, pk2: PackedFilter of [C][C] 1x1 filters; the scales / shifts fp32 [C]
    or None (1 / 0) -> y of a1's shape.  One launch (tlxmi_lka_gate: both products on MFMA, g never in memory) when the "lka" option
    is on, the precision is fp16, the library takes the shape (C a multiple of 32 up to 256) and C <= LKA_GATE_MAX_C; otherwise
    tlxmi_conv2d -> tlxmi_mul -> tlxmi_affine_act -> tlxmi_conv2d (fp32 always: the parity reference).  fused=True / False forces one form (tests, tools/)."""
    need_gpu(a1, "input")
    Cc = a1.shape[-1]
    rows = a1.numel() // Cc
    for o in (t, res):
        if o.shape != a1.shape or o.dtype != a1.dtype or not o.is_contiguous():
            raise RuntimeError(f"lka_gate: a1, t and res must be dense tensors of one shape and dtype, got {tuple(a1.shape)} {a1.dtype} / {tuple(o.shape)} {o.dtype}")
    if not a1.is_contiguous() or any(pk.R != 1 or pk.S != 1 or pk.Cin != Cc or pk.Cout != Cc or pk.dtype != a1.dtype for pk in (pk1, pk2)):
        raise RuntimeError(f"lka_gate: dense operands and two packed {Cc} x {Cc} 1x1 filters of their dtype are expected")
    if fused is None:
        fused = lka_gate_supported(rows, Cc, a1.dtype)
    es = a1.element_size()
    if _sizing():
        _note_act(a1.numel() * es)

    def launch():
        if fused:
            y = torch.empty_like(a1)
            _lib.call("tlxmi_lka_gate", C.byref(_lka_gate_desc(rows, Cc, a1.dtype)), _p(a1), _p(t), _p(pk1.buf), _p(scale1), _p(shift1),
                      _p(pk2.buf), _p(scale2), _p(shift2), _p(res), _p(res_scale), _p(y), _stream())
            return y
        v4 = (lambda v: v) if a1.dim() == 4 else (lambda v: v.view(rows, 1, 1, Cc))
        a2 = conv2d(v4(a1), pk1, 1, 0, 1, scale1, shift1)
        g = mul(v4(t), a2)
        r = affine_act(v4(res), res_scale) if res_scale is not None else v4(res)
        return conv2d(g, pk2, 1, 0, 1, scale2, shift2, res=r).view(a1.shape)
    return _timed(launch, lambda: ((4 * rows * Cc + 2 * Cc * Cc) * es, 4 * rows * Cc * Cc,
                                   (rows, 1, 1, Cc, Cc, "lka_gate" if fused else "conv-mul-affine-conv")))      # the chain is one entry


# ---------------------------------------------------------------------------------------------
# ShuffleNetV2 units
# ---------------------------------------------------------------------------------------------
SHUFFLE_PAD = 8       # a shuffled map of c channels is kept at pitch roundup(c, 8), the columns behind c zero (both dtypes)


def shuffle_pitch(c):
    return (int(c) + SHUFFLE_PAD - 1) // SHUFFLE_PAD * SHUFFLE_PAD


def shuffle_unit_pack(w1, s1, t1, wdw, s2, t2, w2, s3, t3):
    """The parameter image tlxmi_shuffle_unit reads (include/tlxmi.h), as one uint8 tensor on the operands' device: with Kp = h rounded
    up to 32, fp16 w1[Kp][Kp], fp16 w2[Kp][Kp], fp16 wdw[9][Kp] (tap r * 3 + s), fp32 s1, t1, s2, t2, s3, t3 [Kp] each, everything
    beyond h zero.  w1, w2: (h, h, 1, 1) or (h, h) filters (out, in); wdw: (h, 1, 3, 3); the scales / shifts: fp32 [h] (folded BatchNorms)."""
    h = int(w1.shape[0])
    kp = _round_up(h, 32)
    dev = w1.device
    return _param_image(_zero_padded((w1.reshape(h, h), w2.reshape(h, h)), (2, kp, kp), torch.float16, dev), _dw_rsc(wdw, kp, torch.float16, dev),
                        _zero_padded((s1, t1, s2, t2, s3, t3), (6, kp), torch.float32, dev))


class ShuffleUnitParams:
    """One stride-1 InvertedResidual's weights in the forms both arms of shuffle_unit() read: the packed 1x1 filters and the [3][3][hp]
    depthwise filter of the layer-by-layer arm (hp = h rounded up to the dtype's 16-byte chunk, zero filled, as its folded BatchNorm),
    and — fp16, h within the fused kernel — the one-buffer image of tlxmi_shuffle_unit (shuffle_unit_pack)."""

    def __init__(self, w1, bn1, wdw, bn2, w2, bn3, dtype):
        self.h = h = int(w1.shape[0])
        self.dtype = dtype
        self.hp = hp = _round_up(h, vec(dtype))
        (self.s1, self.t1), (s2, t2), (self.s3, self.t3) = ((_f32(a), _f32(b)) for a, b in (bn1, bn2, bn3))
        self.pk1, self.pk2 = PackedFilter(w1, dtype), PackedFilter(w2, dtype)
        self.wdw = _dw_rsc(wdw, hp, dtype, self.s1.device)
        self.s2, self.t2 = _zero_padded(s2, (hp,), torch.float32), _zero_padded(t2, (hp,), torch.float32)
        self.blob = None
        if dtype == torch.float16 and _lib.load().tlxmi_shuffle_unit_param_bytes(h):
            self.blob = shuffle_unit_pack(w1, self.s1, self.t1, wdw, s2, t2, w2, self.s3, self.t3)
            assert self.blob.numel() == _lib.load().tlxmi_shuffle_unit_param_bytes(h)


def _shuffle_unit_desc(x, c, y_ld, act):
    N, H, W, ld = x.shape
    return _lib.ShuffleUnitDesc(dtype=dt_code(x.dtype), N=N, H=H, W=W, C=c, x_ld=ld, y_ld=y_ld, act=act)


# What the fused launch keeps by default is what the library takes (h <= 128): tools/shufflenet_bench.py times each stage shape of x0_5 / x1_0
# against the layer-by-layer arm on one MI355X at batch 256 (profiles/shufflenet/shufflenet_bench_b256.txt), and the fused launch
# won at all five shapes it takes (0.34 - 0.45 of the four launches): there is no routing constant.
def shuffle_unit_supported(x, c=None, act=ACT_RELU, y_ld=None):
    """Whether shuffle_unit() runs tlxmi_shuffle_unit on this NHWC map by default: the "shuffle_unit" option on, fp16 and the
    library takes the shape (h = c / 2 <= 128)."""
    c = x.shape[-1] if c is None else int(c)
    y_ld = shuffle_pitch(c) if y_ld is None else int(y_ld)
    return bool(_options["shuffle_unit"] and x.dtype == torch.float16 and x.is_contiguous()
                and _lib.load().tlxmi_shuffle_unit_supported(C.byref(_shuffle_unit_desc(x, c, y_ld, act))))


def shuffle_concat(a, b, out=None, out_ld=None, cols=None):
    """concat + channel_shuffle(2) of two maps (shufflenetv2.py:75-76): y[..., 2i] = a[..., i], y[..., 2i + 1] = b[..., i] for i < cols
    (default: a's last axis; a and b may be pitched wider) -> y (..., shuffle_pitch(2 cols)) with the columns behind 2 cols zero, or
    written into `out` (pixel pitch out_ld)."""
    need_gpu(a, "input")
    need_gpu(b, "input")
    h = a.shape[-1] if cols is None else int(cols)
    rows = a.numel() // a.shape[-1]
    if a.dtype != b.dtype or not a.is_contiguous() or not b.is_contiguous() or b.numel() // b.shape[-1] != rows or a.shape[-1] < h or b.shape[-1] < h:
        raise RuntimeError(f"shuffle_concat: two dense maps of one dtype with the same pixels and at least {h} channels are expected, got "
                           f"{tuple(a.shape)} {a.dtype} / {tuple(b.shape)} {b.dtype}")
    if out is None:
        out_ld = shuffle_pitch(2 * h)
        out = torch.empty(tuple(a.shape[:-1]) + (out_ld,), dtype=a.dtype, device=a.device)
    elif out_ld is None:
        out_ld = out.shape[-1]
    if out.dtype != a.dtype or out_ld < 2 * h:
        raise RuntimeError("shuffle_concat: out must have the operands' dtype and a pitch of at least twice their channels")
    es = a.element_size()
    if _sizing():
        _note_act(a.numel() * es, b.numel() * es, rows * out_ld * es)
    _lib.call("tlxmi_shuffle_concat", _p(a), _p(b), _p(out), dt_code(a.dtype), rows, h, a.shape[-1], b.shape[-1], out_ld, _stream())
    return out


def shuffle_unit(x, params, act, fused=None, out=None):
    """ShuffleNetV2's stride-1 InvertedResidual (shufflenetv2.py:69-76) on an NHWC map x (N, H, W, x_ld) whose first c = 2 h channels are
    the input (h = params.h): the second half runs 1x1 + BN + act -> depthwise 3x3 + BN -> 1x1 + BN + act, the maps between them rounded
    to the activation dtype, and is interleaved with the untouched first half -> y (N, H, W, shuffle_pitch(c)), the columns behind c zero,
    or written into `out` (its last axis is the pitch).  params: ShuffleUnitParams.  One launch (tlxmi_shuffle_unit, the hidden maps in
    LDS) when the "shuffle_unit" option is on, the precision is fp16 and the library takes the shape (h <= 128); otherwise tlxmi_conv2d ->
    tlxmi_dwconv2d -> tlxmi_conv2d -> tlxmi_shuffle_concat (fp32 always: the parity reference), the branch half copied out first where
    it does not start on a 16-byte boundary.  fused=True / False forces one form (tests, tools/); True raises where the launch is not
    supported."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    h = params.h
    c = 2 * h
    if x.dtype != params.dtype or ld < c or not x.is_contiguous():
        raise RuntimeError(f"shuffle_unit: x must be a dense NHWC map of the parameters' dtype with at least {c} channels, got {tuple(x.shape)} {x.dtype}")
    out, y_ld = _out_map("shuffle_unit", out, N, H, W, c, x.dtype, x.device, shuffle_pitch(c),
                         what="a dense map of x's dtype and pixels with at least c channels")
    desc = _shuffle_unit_desc(x, c, y_ld, act)
    takes = bool(x.dtype == torch.float16 and params.blob is not None and _lib.load().tlxmi_shuffle_unit_supported(C.byref(desc)))
    fused = _use_fused("shuffle_unit", fused, takes, takes and _options["shuffle_unit"],
                       lambda: f"{tuple(x.shape)} {x.dtype} with h = {h}, act {act}, y_ld {y_ld}")
    es = x.element_size()
    M = N * H * W
    if _sizing():
        _note_act(x.numel() * es, M * y_ld * es)

    def launch():
        if fused:
            _lib.call("tlxmi_shuffle_unit", C.byref(desc), _p(x), _p(params.blob), _p(out), _stream())
            return
        v, hp = vec(x.dtype), params.hp
        if h % v == 0 and ld % v == 0:
            t = _conv2d(x[..., h:c], params.pk1, 1, 0, 1, params.s1, params.t1, act=act, x_ld=ld)
        else:       # the branch half starts inside a 16-byte chunk: a dense copy, zero filled up to the filter's padded width
            xb = torch.zeros((N, H, W, hp), dtype=x.dtype, device=x.device)
            xb[..., :h] = x[..., h:c]
            t = torch.zeros((N, H, W, hp), dtype=x.dtype, device=x.device)      # (its pad columns feed the depthwise: zeros)
            _conv2d(xb, params.pk1, 1, 0, 1, params.s1, params.t1, act=act, out=t, out_ld=hp)
        t = dwconv2d(t, params.wdw, 1, 1, 1, params.s2, params.t2)
        f = torch.empty((N, H, W, hp), dtype=x.dtype, device=x.device)
        _conv2d(t, params.pk2, 1, 0, 1, params.s3, params.t3, act=act, out=f, out_ld=hp)
        shuffle_concat(x, f, out, y_ld, cols=h)
    _timed(launch, lambda: ((2 * M * c + 2 * h * h + 9 * h) * es, 2 * M * h * (2 * h + 9),
                            (N, H, W, c, c, "shuffle_unit" if fused else "conv-dw-conv-shuffle")))      # the chain is one entry
    return out


# ---------------------------------------------------------------------------------------------
# GhostNet's Ghost module
# ---------------------------------------------------------------------------------------------
def ghost_module_pack(w1, s1, t1, wdw, s2, t2):
    """The parameter image tlxmi_ghost_module reads (include/tlxmi.h), as one uint8 tensor on the operands' device: with Kp = Cin
    rounded up to 32 and mp = m rounded up to 16, fp16 w1[mp][Kp], fp16 wdw[9][mp] (tap r * 3 + s), fp32 s1, t1, s2, t2 [mp] each,
    everything beyond Cin / m zero.  w1: (m, Cin, 1, 1) or (m, Cin) (out, in); wdw: (m, 1, 3, 3); the scales / shifts: fp32 [m]
    (folded BatchNorms)."""
    m, cin = int(w1.shape[0]), int(w1.shape[1])
    kp, mp = _round_up(cin, 32), _round_up(m, 16)
    dev = w1.device
    return _param_image(_zero_padded(w1.reshape(m, cin), (mp, kp), torch.float16), _dw_rsc(wdw, mp, torch.float16, dev),
                        _zero_padded((s1, t1, s2, t2), (4, mp), torch.float32, dev))


class GhostModuleParams:
    """One GhostModule's weights in the forms both arms of ghost_module() read: the packed 1x1 filter and the [3][3][mp] depthwise
    filter of the layer-by-layer arm (mp = m rounded up to the dtype's 16-byte chunk, zero filled, as its folded BatchNorm), and — fp16,
    widths within the fused kernel — the one-buffer image of tlxmi_ghost_module (ghost_module_pack).  w1: (m, Cin, 1, 1);
    wdw: (m, 1, 3, 3); bn1, bn2: (scale, shift) of the folded BatchNorms."""

    def __init__(self, w1, bn1, wdw, bn2, dtype):
        self.m = m = int(w1.shape[0])
        self.cin = int(w1.shape[1])
        self.dtype = dtype
        self.mp = mp = _round_up(m, vec(dtype))
        (self.s1, self.t1), (s2, t2) = ((_f32(a), _f32(b)) for a, b in (bn1, bn2))
        self.pk1 = PackedFilter(w1, dtype)
        self.wdw = _dw_rsc(wdw, mp, dtype, self.s1.device)
        self.s2, self.t2 = _zero_padded(s2, (mp,), torch.float32), _zero_padded(t2, (mp,), torch.float32)
        self.blob = None
        if dtype == torch.float16 and _lib.load().tlxmi_ghost_module_param_bytes(self.cin, m):
            self.blob = ghost_module_pack(w1, self.s1, self.t1, wdw, s2, t2)
            assert self.blob.numel() == _lib.load().tlxmi_ghost_module_param_bytes(self.cin, m)


def _ghost_module_desc(x, cin, m, y_ld, res_ld, act):
    N, H, W, ld = x.shape
    return _lib.GhostModuleDesc(dtype=dt_code(x.dtype), N=N, H=H, W=W, Cin=cin, m=m, x_ld=ld, y_ld=y_ld, res_ld=res_ld, act=act)


def ghost_module_takes(x, cin, m, act=ACT_RELU, y_ld=None, res_ld=0):
    """Whether the library's tlxmi_ghost_module takes this NHWC map (fp16, widths and pitches within the kernel): what fused=True needs."""
    y_ld = shuffle_pitch(2 * m) if y_ld is None else int(y_ld)
    return bool(x.dtype == torch.float16 and x.is_contiguous()
                and _lib.load().tlxmi_ghost_module_supported(C.byref(_ghost_module_desc(x, int(cin), int(m), y_ld, int(res_ld), act))))


# Which shapes the fused launch keeps by default.  MEASURED: tools/ghostnet_bench.py times every distinct module shape of ghostnet_x0_5 /
# ghostnet_x1_0 against the layer-by-layer arm on one MI355X at batch 256 (profiles/ghostnet/ghostnet_bench_b256.txt).  The
# fused launch won (0.44 - 0.92 of the layers' time) at every shape with a map of at most 56 x 56, m <= 100 and Cin * m <= 19200, and
# lost (1.16 - 2.41) at every other one: the 112 x 112 maps (4 - 24 channels on a 16 x 32 MFMA tile), m >= 120 (two or more channel
# chunks, each recomputing the halo and re-reading x) and Cin >= 480 with m >= 56 (filter rows that leave LDS room for 16 - 48
# channels a chunk).  The three bounds are the table's, not a model: shapes between its rows (x1_3, other resolutions) are unmeasured.
GHOST_FUSED_MAX_PIXELS, GHOST_FUSED_MAX_M, GHOST_FUSED_MAX_CIN_M = 56 * 56, 100, 19200


def _ghost_module_routed(H, W, cin, m):
    return H * W <= GHOST_FUSED_MAX_PIXELS and m <= GHOST_FUSED_MAX_M and cin * m <= GHOST_FUSED_MAX_CIN_M


def ghost_module_supported(x, cin, m, act=ACT_RELU, y_ld=None, res_ld=0):
    """Whether ghost_module() runs tlxmi_ghost_module on this NHWC map by default: the "ghost_module" option on, the library takes the
    shape (ghost_module_takes) and the measured table keeps it (otherwise it runs layer by layer)."""
    return bool(_options["ghost_module"] and _ghost_module_routed(x.shape[1], x.shape[2], int(cin), int(m))
                and ghost_module_takes(x, cin, m, act, y_ld, res_ld))


def ghost_module(x, params, act, res=None, fused=None, out=None):
    """GhostNet's GhostModule (ghostnet.py:74-94) on an NHWC map x (N, H, W, x_ld) whose first Cin = params.cin channels are the input:
    primary = act(1x1 * s1 + t1) (m = params.m channels), cheap = act(dw3x3(primary rounded to the activation dtype) * s2 + t2),
    y = concat([primary, cheap]) (+ res, the bottleneck's shortcut, ghostnet.py:140; a map of the same pixels with at least 2 m
    channels, which may be x) -> y (N, H, W, shuffle_pitch(2 m)), the columns behind 2 m zero, or written into `out` (its last axis
    is the pitch).  params: GhostModuleParams.  One launch (tlxmi_ghost_module, the primary map in LDS) when the "ghost_module"
    option is on, the precision is fp16, the library takes the shape and the measured table keeps it (ghost_module_supported); otherwise tlxmi_conv2d into out[..., :m] -> tlxmi_dwconv2d
    from there into out[..., m:] (through a dense copy where m is no whole number of 16-byte chunks) -> tlxmi_affine_act for the
    shortcut (fp32 always: the parity reference; there the pitches are whole chunks and res has zero pad columns).  fused=True /
    False forces one form (tests, tools/); True raises where the launch is not supported."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    m, cin = params.m, params.cin
    c = 2 * m
    if x.dtype != params.dtype or ld < cin or not x.is_contiguous():
        raise RuntimeError(f"ghost_module: x must be a dense NHWC map of the parameters' dtype with at least {cin} channels, got {tuple(x.shape)} {x.dtype}")
    out, y_ld = _out_map("ghost_module", out, N, H, W, c, x.dtype, x.device, shuffle_pitch(c),
                         what="a dense map of x's dtype and pixels with at least 2 m channels")
    res_ld = 0
    if res is not None:
        res_ld = res.shape[-1]
        if res.dtype != x.dtype or tuple(res.shape[:3]) != (N, H, W) or res_ld < c or not res.is_contiguous():
            raise RuntimeError("ghost_module: res must be a dense map of x's dtype and pixels with at least 2 m channels")
    desc = _ghost_module_desc(x, cin, m, y_ld, res_ld, act)
    takes = bool(x.dtype == torch.float16 and params.blob is not None and _lib.load().tlxmi_ghost_module_supported(C.byref(desc)))
    fused = _use_fused("ghost_module", fused, takes, lambda: takes and _options["ghost_module"] and _ghost_module_routed(H, W, cin, m),
                       lambda: f"{tuple(x.shape)} {x.dtype} with Cin = {cin}, m = {m}, act {act}, y_ld {y_ld}, res_ld {res_ld}")
    es = x.element_size()
    M = N * H * W
    if _sizing():
        _note_act(x.numel() * es, M * y_ld * es, M * res_ld * es)

    def launch():
        if fused:
            _lib.call("tlxmi_ghost_module", C.byref(desc), _p(x), _p(params.blob), _p(res), _p(out), _stream())
            return
        v, mp = vec(x.dtype), params.mp
        zend = min(y_ld, shuffle_pitch(c))
        if ld < params.pk1.Cin_pad:
            raise RuntimeError(f"ghost_module: layer by layer, x needs a pitch of at least {params.pk1.Cin_pad} channels")
        if m % v == 0 and y_ld % v == 0:
            _conv2d(x, params.pk1, 1, 0, 1, params.s1, params.t1, act=act, out=out, out_ld=y_ld)
            dwconv2d(out[..., :m], params.wdw, 1, 1, 1, params.s2, params.t2, act=act, x_ld=y_ld, out=out[..., m:], out_ld=y_ld)
        else:       # the cheap half starts inside a 16-byte chunk: dense copies, zero filled up to the filter's padded width
            t = torch.zeros((N, H, W, mp), dtype=x.dtype, device=x.device)
            _conv2d(x, params.pk1, 1, 0, 1, params.s1, params.t1, act=act, out=t, out_ld=mp)
            u = dwconv2d(t, params.wdw, 1, 1, 1, params.s2, params.t2, act=act)
            out[..., :m] = t[..., :m]
            out[..., m:c] = u[..., :m]
        if zend > c:
            out[..., c:zend] = 0
        if res is not None:
            cw = (c + v - 1) // v * v
            if cw > zend or y_ld % v or res_ld % v or res_ld < cw:
                raise RuntimeError(f"ghost_module: layer by layer, the shortcut needs pitches that are whole 16-byte chunks (y_ld {y_ld}, res_ld {res_ld})")
            _lib.call("tlxmi_affine_act", _p(out), None, None, _p(res), _p(out), dt_code(x.dtype), M, cw, y_ld, res_ld, y_ld, ACT_NONE, 0.0, 0,
                      _stream())
    _timed(launch, lambda: ((M * (cin + c * (2 if res is not None else 1)) + m * cin + 9 * m) * es, 2 * M * m * (cin + 9),
                            (N, H, W, cin, c, "ghost_module" if fused else "conv-dw-add")))      # the chain is one entry
    return out


# ---------------------------------------------------------------------------------------------
# MixNet's mixed depthwise convolution
# ---------------------------------------------------------------------------------------------
def mixconv_dw_pack(filters, scale, shift, dtype):
    """The parameter image tlxmi_mixconv_dw reads (include/tlxmi.h), as one uint8 tensor on the operands' device.  filters: one
    (n_g, 1, k_g, k_g) tensor a group, in channel order; scale / shift: fp32 [C] (the folded BatchNorm over the concatenated map).
    With kmax the largest k_g: T w[C / 8][kmax * kmax][8] — slab s (channels 8 s .. 8 s + 7) runs at K_s, the largest window among
    its channels, and its first K_s * K_s * 8 entries are [K_s][K_s][8]; a channel with a smaller window sits centred among zero
    taps — then fp32 scale[C], shift[C]."""
    ks = [int(f.shape[-1]) for f in filters]
    ns = [int(f.shape[0]) for f in filters]
    Cc, kmax = sum(ns), max(ks)
    dev = filters[0].device
    kc = torch.cat([torch.full((n,), k, dtype=torch.int64) for n, k in zip(ns, ks)])          # window of every channel
    full = torch.zeros((Cc, kmax, kmax), dtype=torch.float32, device=dev)                     # every channel centred at kmax
    a = 0
    for f, n, k in zip(filters, ns, ks):
        o = (kmax - k) // 2
        full[a:a + n, o:o + k, o:o + k] = f.detach().reshape(n, k, k).to(torch.float32)
        a += n
    w = torch.zeros((Cc // 8, kmax * kmax, 8), dtype=dtype, device=dev)
    for s in range(Cc // 8):
        K = int(kc[8 * s:8 * s + 8].max())
        o = (kmax - K) // 2
        w[s, :K * K] = full[8 * s:8 * s + 8, o:o + K, o:o + K].reshape(8, K * K).t().to(dtype)
    return _param_image(w, torch.stack([scale.detach().to(torch.float32), shift.detach().to(torch.float32)]))


class MixConvParams:
    """One MixConv's weights in the forms both arms of mixconv_dw() read: a group's [k][k][n_g] depthwise filter and its slice of the
    folded BatchNorm for tlxmi_dwconv2d (padded with zeros to whole 16-byte chunks where n_g is none), and — C a multiple of 8, at
    most five groups, odd windows 3 .. 11 — the one-buffer image of tlxmi_mixconv_dw (mixconv_dw_pack).  filters: one (n_g, 1, k_g, k_g)
    tensor a group; bn: (scale, shift) fp32 [C] over the concatenated channels."""

    def __init__(self, filters, bn, dtype):
        self.groups = [int(f.shape[0]) for f in filters]
        self.kernels = [int(f.shape[-1]) for f in filters]
        self.C = sum(self.groups)
        self.dtype = dtype
        self.scale, self.shift = _f32(bn[0]), _f32(bn[1])
        dev = self.scale.device
        v = vec(dtype)
        self.per_group = []
        a = 0
        for f, n, k in zip(filters, self.groups, self.kernels):
            npad = _round_up(n, v)
            s, t = _zero_padded(self.scale[a:a + n], (npad,), torch.float32), _zero_padded(self.shift[a:a + n], (npad,), torch.float32)
            self.per_group.append((a, n, npad, _dw_rsc(f, npad, dtype, dev), s, t))
            a += n
        self.blob = None
        in_range = (self.C % 8 == 0 and 1 <= len(filters) <= 5 and all(3 <= k <= 11 and k % 2 for k in self.kernels)
                    and all(tuple(f.shape[1:]) == (1, k, k) for f, k in zip(filters, self.kernels)))
        if in_range:
            self.blob = mixconv_dw_pack([f.to(dev) for f in filters], self.scale, self.shift, dtype)
            assert self.blob.numel() == _lib.load().tlxmi_mixconv_dw_param_bytes(C.byref(_mixconv_desc(
                dtype, 1, 1, 1, self.C, self.groups, self.kernels, 1, self.C, self.C, self.C, ACT_NONE)))


def _mixconv_desc(dtype, N, H, W, Cc, groups, kernels, stride, x_ld, y_ld, pool_ld, act):
    d = _lib.MixConvDwDesc(dtype=dt_code(dtype), N=N, H=H, W=W, C=Cc, G=len(groups), stride=stride, x_ld=x_ld, y_ld=y_ld, pool_ld=pool_ld, act=act)
    for i in range(min(len(groups), 5)):
        d.group_channels[i], d.kernel[i] = int(groups[i]), int(kernels[i])
    return d


def mixconv_dw_supported(x, groups, kernels, stride=1, act=ACT_NONE, pool=False, y_ld=None):
    """Whether mixconv_dw() runs tlxmi_mixconv_dw on this NHWC map by default: the "mixconv" option on and the library takes the
    shape (fp16 or fp32; C = sum(groups) a multiple of 8; at most five groups, odd windows 3 .. 11; stride 1 or 2; pitches in whole
    16-byte chunks; with pool, the padded 8-channel slab of an image within the LDS — include/tlxmi.h).  More than five groups, a
    stride pair or an activation code outside the descriptor are simply not taken."""
    groups, kernels = list(groups), list(kernels)
    if not _options["mixconv"] or x.dim() != 4 or not x.is_contiguous() or x.dtype not in (torch.float16, torch.float32):
        return False
    if len(groups) != len(kernels) or not 1 <= len(groups) <= 5 or not isinstance(stride, int):
        return False
    N, H, W, ld = x.shape
    Cc = sum(groups)
    y_ld = Cc if y_ld is None else int(y_ld)
    return bool(_lib.load().tlxmi_mixconv_dw_supported(C.byref(_mixconv_desc(x.dtype, N, H, W, Cc, groups, kernels, stride, ld, y_ld, Cc, act)),
                                                       1 if pool else 0))


def mixconv_dw(x, params, stride, act, pool=False, fused=None, out=None):
    """MixNet's MixConv + BatchNorm + activation (mixnet.py:244-252, :308-314) on an NHWC map x (N, H, W, x_ld) whose first
    C = params.C channels are the input: channel c of group g runs a depthwise k_g x k_g conv (pad (k_g - 1) / 2, `stride`), then
    * scale + shift and act -> y (N, Ho, Wo, C), or written into `out` (its last axis is the pitch; nothing behind C is written).
    pool=True also returns the Squeeze-Excitation pool of y, (N, C) in x's dtype: -> (y, pool).  One launch (tlxmi_mixconv_dw) when
    the "mixconv" option is on and the library takes the shape (mixconv_dw_supported); otherwise one tlxmi_dwconv2d a group — on the
    column slice where it starts and ends on 16-byte chunks, through a dense zero-padded copy of the slice otherwise — and
    tlxmi_global_avgpool.  fused=True / False forces one form (tests, tools/); True raises where the launch is not supported."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    Cc = params.C
    if x.dtype != params.dtype or ld < Cc or not x.is_contiguous():
        raise RuntimeError(f"mixconv_dw: x must be a dense NHWC map of the parameters' dtype with at least {Cc} channels, got {tuple(x.shape)} {x.dtype}")
    if not isinstance(stride, int) or stride < 1:
        raise RuntimeError(f"mixconv_dw: one positive stride for both axes, got {stride!r}")
    extents = {((H + 2 * ((k - 1) // 2) - k) // stride + 1, (W + 2 * ((k - 1) // 2) - k) // stride + 1) for k in params.kernels}
    if len(extents) != 1 or min(extents.pop()) < 1:
        raise RuntimeError(f"mixconv_dw: windows {params.kernels} at pad (k - 1) // 2 do not give one output extent on {H} x {W}")
    k0 = params.kernels[0]
    Ho, Wo = (H + 2 * ((k0 - 1) // 2) - k0) // stride + 1, (W + 2 * ((k0 - 1) // 2) - k0) // stride + 1
    out, y_ld = _out_map("mixconv_dw", out, N, Ho, Wo, Cc, x.dtype, x.device, Cc, what=f"a dense ({N}, {Ho}, {Wo}, >= {Cc}) map of x's dtype")
    desc = _mixconv_desc(x.dtype, N, H, W, Cc, params.groups, params.kernels, stride, ld, y_ld, Cc, act)
    takes = bool(params.blob is not None and _lib.load().tlxmi_mixconv_dw_supported(C.byref(desc), 1 if pool else 0))
    fused = _use_fused("mixconv_dw", fused, takes, takes and _options["mixconv"],
                       lambda: f"{tuple(x.shape)} {x.dtype} with groups {params.groups}, windows {params.kernels}, stride {stride}, act {act}, "
                               f"y_ld {y_ld}, pool {pool}")
    es = x.element_size()
    if _sizing():
        _note_act(x.numel() * es, out.numel() * es)
    pooled = torch.empty((N, Cc), dtype=x.dtype, device=x.device) if pool else None

    def launch():
        if fused:
            _lib.call("tlxmi_mixconv_dw", C.byref(desc), _p(x), _p(params.blob), _p(out), _p(pooled), _stream())
            return
        v = vec(x.dtype)
        for (a, n, npad, w, s, t), k in zip(params.per_group, params.kernels):
            if a % v == 0 and n % v == 0 and ld % v == 0 and y_ld % v == 0:
                dwconv2d(x[..., a:a + n], w, stride, (k - 1) // 2, 1, s, t, act=act, x_ld=ld, out=out[..., a:a + n], out_ld=y_ld)
            else:       # the slice starts or ends inside a 16-byte chunk: a dense copy, zero filled up to the filter's padded width
                piece = torch.zeros((N, H, W, npad), dtype=x.dtype, device=x.device)
                piece[..., :n] = x[..., a:a + n]
                out[..., a:a + n] = dwconv2d(piece, w, stride, (k - 1) // 2, 1, s, t, act=act)[..., :n]
        if pool and Cc % v == 0 and y_ld % v == 0:
            _lib.call("tlxmi_global_avgpool", _p(out), _p(pooled), dt_code(x.dtype), N, Ho * Wo, Cc, y_ld, Cc, _stream())
        elif pool:      # C or the pitch is no whole number of 16-byte chunks: pool a dense zero-padded copy
            cp = (Cc + v - 1) // v * v
            wide = torch.zeros((N, Ho, Wo, cp), dtype=x.dtype, device=x.device)
            wide[..., :Cc] = out[..., :Cc]
            pooled.copy_(global_avgpool(wide)[:, :Cc])

    def entry():
        taps = sum(n * k * k for n, k in zip(params.groups, params.kernels))
        return (N * H * W * Cc + N * Ho * Wo * Cc + taps) * es, 2 * N * Ho * Wo * taps, (N, H, W, Cc, Cc, "mixconv_dw" if fused else "dw-per-group")
    _timed(launch, entry)      # the chain is one entry
    return (out, pooled) if pool else out


# ---------------------------------------------------------------------------------------------
# Res2Net's hierarchical 3x3 chain
# ---------------------------------------------------------------------------------------------
def res2_chain_pack(filters, bns, w):
    """The parameter image tlxmi_res2_chain reads (include/tlxmi.h), as one uint8 tensor on the operands' device.  filters: one
    (w, w, 3, 3) tensor a conv, in chain order; bns: one (scale, shift) fp32 [w] pair a conv.  np = w rounded up to 16, kp = w rounded
    up to 32: fp16 filt[nc][9][np][kp] (tap r * 3 + s, row = output channel, column = input channel, zero padded), then fp32
    scale[nc][np], shift[nc][np]."""
    nc, dev = len(filters), filters[0].device
    np_, kp = _round_up(w, 16), _round_up(w, 32)
    taps = [wt.detach().to(torch.float32).permute(2, 3, 0, 1).reshape(9, w, w) for wt in filters]
    return _param_image(_zero_padded(taps, (nc, 9, np_, kp), torch.float16, dev),
                        _zero_padded([sc for sc, _ in bns] + [sh for _, sh in bns], (2 * nc, np_), torch.float32, dev))


class Res2ChainParams:
    """The 3x3 convs of one Res2Net block (scales - 1 of them, w -> w channels each) in the forms both arms of res2_chain() read: a conv's
    filter zero-padded to wp x wp channels (PackedFilter) with its folded BatchNorm zero-padded to wp, for tlxmi_conv2d on a slice of
    the padded map; and — fp16, 2 <= scales <= 8, 8 <= w <= 208, w <= wp <= roundup(w, 16) — the one-buffer image of tlxmi_res2_chain
    (res2_chain_pack).  filters: one (w, w, 3, 3) tensor a conv; bns: one (scale, shift) fp32 [w] pair a conv; wp: the slice pitch, a
    multiple of 8."""

    def __init__(self, filters, bns, w, wp, dtype):
        if len(filters) != len(bns) or not filters or wp < w or wp % 8 or any(tuple(f.shape) != (w, w, 3, 3) for f in filters):
            raise RuntimeError(f"Res2ChainParams: {len(filters)} filters of (w, w, 3, 3) with w = {w}, as many (scale, shift) pairs and a pitch "
                               f"wp >= w that is a multiple of 8 are expected, got wp = {wp}, {[tuple(f.shape) for f in filters]}")
        self.w, self.wp, self.scales, self.dtype = int(w), int(wp), len(filters) + 1, dtype
        dev = filters[0].device
        self.per_conv = []
        for wt, (sc, sh) in zip(filters, bns):
            full = _zero_padded(wt, (wp, wp, 3, 3), torch.float32, dev)
            self.per_conv.append((PackedFilter(full, dtype), _zero_padded(_f32(sc), (wp,), torch.float32, dev), _zero_padded(_f32(sh), (wp,), torch.float32, dev)))
        self.blob = None
        d = _res2_chain_desc(dtype, 1, 1, 1, self.w, self.wp, self.scales, self.scales * self.wp, self.scales * self.wp, ACT_NONE) \
            if dtype == torch.float16 else None
        if d is not None and _lib.load().tlxmi_res2_chain_supported(C.byref(d)):
            self.blob = res2_chain_pack([f.to(dev) for f in filters], [(_f32(a), _f32(b)) for a, b in bns], self.w)
            assert self.blob.numel() == _lib.load().tlxmi_res2_chain_param_bytes(C.byref(d))


def _res2_chain_desc(dtype, N, H, W, w, wp, scales, x_ld, y_ld, act):
    return _lib.Res2ChainDesc(dtype=dt_code(dtype), N=N, H=H, W=W, w=w, wp=wp, scales=scales, x_ld=x_ld, y_ld=y_ld, act=act)


def res2_chain_takes(x, w, wp, scales, act=ACT_RELU, y_ld=None):
    """Whether tlxmi_res2_chain takes this NHWC map (the library's predicate: include/tlxmi.h)."""
    if x.dim() != 4 or not x.is_contiguous() or x.dtype != torch.float16:
        return False
    N, H, W, ld = x.shape
    y_ld = scales * wp if y_ld is None else int(y_ld)
    return bool(_lib.load().tlxmi_res2_chain_supported(C.byref(_res2_chain_desc(x.dtype, N, H, W, w, wp, scales, ld, y_ld, act))))


# (H, W, w, scales) of the chains where the one launch was measured FASTER than the layer-by-layer arm beyond the spread of both, at batch
# 256 on one MI355X (tools/res2net_bench.py, profiles/res2net/res2net_bench_b256.txt): res2_chain() keeps the launch there and runs the
# layered arm everywhere else by default.  The launch wins where w <= 32 — a conv's filter fragments stay in registers — and the map is
# large: 0.86 of the layered time at Res2Net-50 26w x 4s's 56 x 56 blocks, 0.85 / 0.43 at 14w x 8s's 56 x 56 / 28 x 28 blocks; it takes
# 1.7 - 3.0 x the layered time at the wider slices of the later stages (DESIGN 4.29 says why)
RES2_CHAIN_WINS = frozenset({(56, 56, 26, 4), (56, 56, 14, 8), (28, 28, 28, 8)})


def _res2_chain_routed(H, W, w, scales):
    return (H, W, w, scales) in RES2_CHAIN_WINS


def res2_chain_supported(x, w, wp, scales, act=ACT_RELU, y_ld=None):
    """Whether res2_chain() runs tlxmi_res2_chain on this map by default: the "res2chain" option on, the library takes the shape
    (res2_chain_takes) and the measured table keeps it (RES2_CHAIN_WINS)."""
    return bool(_options["res2chain"] and x.dim() == 4 and _res2_chain_routed(x.shape[1], x.shape[2], w, scales)
                and res2_chain_takes(x, w, wp, scales, act, y_ld))


def res2_chain(x, params, act, fused=None, out=None):
    """The hierarchical 3x3 chain of a stride-1 Res2Net block (res2net.py:76-90) on an NHWC map x (N, H, W, x_ld) whose slice s is the
    columns [s wp, s wp + w): y_0 = act(bn_0(conv_0(x_0))), y_s = act(bn_s(conv_s(x_s + y_{s-1}))), the last slice passes through
    -> y (N, H, W, scales * wp), or written into `out` (its last axis is the pitch; nothing behind scales * wp is written), the pad
    columns [s wp + w, (s + 1) wp) zero.  One launch (tlxmi_res2_chain) when the "res2chain" option is on, the library takes the shape
    and the measured table keeps it (res2_chain_supported); otherwise — and for fp32 — tlxmi_conv2d on a slice, tlxmi_affine_act with
    res (the add) into a dense scratch slice, tlxmi_conv2d ... and tlxmi_copy_channels for the last slice.  The layered arm reads the
    pad columns of x through zero filter columns, so they must be finite there (the reduce conv of the model writes zeros).
    fused=True / False forces one form (tests, tools/); True raises where the launch is not supported."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    w, wp, S = params.w, params.wp, params.scales
    if x.dtype != params.dtype or ld < S * wp or ld % 8 or not x.is_contiguous():
        raise RuntimeError(f"res2_chain: x must be a dense NHWC map of the parameters' dtype with at least {S * wp} channels at a pitch that "
                           f"is a multiple of 8, got {tuple(x.shape)} {x.dtype}")
    out, y_ld = _out_map("res2_chain", out, N, H, W, S * wp, x.dtype, x.device, S * wp, multiple=8,
                         what=f"a dense ({N}, {H}, {W}, >= {S * wp}) map of x's dtype at a pitch that is a multiple of 8")
    takes = lambda: params.blob is not None and res2_chain_takes(x, w, wp, S, act, y_ld)      # noqa: E731
    # the option and the table first: the library's predicate is asked only where they keep the launch
    fused = _use_fused("res2_chain", fused, takes, lambda: _options["res2chain"] and _res2_chain_routed(H, W, w, S) and takes(),
                       lambda: f"{tuple(x.shape)} {x.dtype} with w {w}, wp {wp}, scales {S}, act {act}, y_ld {y_ld}")
    es = x.element_size()
    if _sizing():
        _note_act(x.numel() * es, out.numel() * es)

    def launch():
        if fused:
            desc = _res2_chain_desc(x.dtype, N, H, W, w, wp, S, ld, y_ld, act)
            _lib.call("tlxmi_res2_chain", C.byref(desc), _p(x), _p(params.blob), _p(out), _stream())
            return
        rows, dt = N * H * W, dt_code(x.dtype)
        scratch = torch.empty((N, H, W, wp), dtype=x.dtype, device=x.device) if S > 2 else None
        for j, (pk, s, t) in enumerate(params.per_conv):
            dst = out[..., j * wp:(j + 1) * wp]
            if j == 0:
                conv2d(x[..., :wp], pk, 1, 1, 1, s, t, act=act, out=dst, out_ld=y_ld, x_ld=ld)
            else:       # a_j = x_j + y_{j-1}: the add comes BEFORE the conv, so it cannot ride a conv epilogue
                _lib.call("tlxmi_affine_act", _p(x[..., j * wp:(j + 1) * wp]), _p(None), _p(None), _p(out[..., (j - 1) * wp:j * wp]), _p(scratch),
                          dt, rows, wp, ld, y_ld, wp, ACT_NONE, 0.0, 0, _stream())
                conv2d(scratch, pk, 1, 1, 1, s, t, act=act, out=dst, out_ld=y_ld)
        _lib.call("tlxmi_copy_channels", _p(x[..., (S - 1) * wp:S * wp]), _p(out[..., (S - 1) * wp:S * wp]), dt, rows, wp, ld, y_ld, _stream())
    _timed(launch, lambda: ((2 * N * H * W * S * w + (S - 1) * 9 * w * w) * es, 2 * N * H * W * (S - 1) * 9 * w * w,
                            (N, H, W, S * w, S * w, "res2_chain" if fused else "conv-add-conv-copy")))      # the chain is one entry
    return out


# ---------------------------------------------------------------------------------------------
# GoogLeNet's Inception module: the branches that read x
# ---------------------------------------------------------------------------------------------
def inception_head_pack(w1, w3r, w5r, wp):
    """The parameter image tlxmi_inception_head reads (include/tlxmi.h), as one uint8 tensor on the operands' device: fp16 [R][Kp], the
    rows of the four 1x1 filters in the order W1, W3r, W5r, Wp, each padded with zero rows to a multiple of 16, Kp = Cin rounded up
    to 64, zero behind Cin.  Each filter: (out, Cin, 1, 1) or (out, Cin)."""
    cin = int(w1.shape[1])
    kp = _round_up(cin, 64)
    return _param_image(*[_zero_padded(w.reshape(w.shape[0], cin), (_round_up(w.shape[0], 16), kp), torch.float16, w1.device)
                          for w in (w1, w3r, w5r, wp)])


class InceptionParams:
    """The four 1x1 filters of one Inception module that read its input, in the forms both arms of inception_head() read: a
    PackedFilter each for the layer-by-layer arm, and — fp16 — the one-buffer image of tlxmi_inception_head (inception_head_pack).
    w1, w3r, w5r, wp: (f1 | f3R | f5R | proj, Cin, 1, 1); f3, f5: the widths of the module's 3x3 and 5x5 convs, whose slices of the
    output lie between w1's and wp's.  The slices of the output map y are [0, f1) | [o3, o3 + f3) | [o5y, o5y + f5) | [op, op + proj)
    = the concatenation of the reference (googlenet.py:63); the mid map t holds the 3x3 reduce map at [0, f3R) and the 5x5 one at
    [t5, t5 + f5R), t5 = f3R rounded up to 8, at pitch t_ld = t5 + f5R.  Every width must be a multiple of 8 (each slice then starts
    on a 16-byte boundary in both dtypes; all nine modules of GoogLeNet do): other widths are REFUSED here, in both arms.
    t5: another offset of the 5x5 reduce map in the mid map (a multiple of 8, at least f3R; tests)."""

    def __init__(self, w1, w3r, w5r, wp, f3, f5, dtype, t5=None):
        self.cin = int(w1.shape[1])
        self.f1, self.f3r, self.f5r, self.proj, self.f3, self.f5 = (int(w1.shape[0]), int(w3r.shape[0]), int(w5r.shape[0]), int(wp.shape[0]),
                                                                    int(f3), int(f5))
        widths = (self.cin, self.f1, self.f3r, self.f5r, self.proj, self.f3, self.f5)
        if any(int(w.shape[1]) != self.cin for w in (w3r, w5r, wp)) or any(n <= 0 or n % 8 for n in widths):
            raise RuntimeError(f"InceptionParams: four 1x1 filters over the same Cin are expected, and Cin and every width a multiple of 8 "
                               f"(a slice of the output map must start on a 16-byte boundary); got Cin / f1 / f3R / f5R / proj / f3 / f5 = {widths}")
        self.dtype = dtype
        self.o3, self.o5y, self.op = self.f1, self.f1 + self.f3, self.f1 + self.f3 + self.f5
        self.cout = self.op + self.proj
        self.t5 = _round_up(self.f3r, 8) if t5 is None else int(t5)
        if self.t5 < self.f3r or self.t5 % 8:
            raise RuntimeError(f"InceptionParams: t5 must be a multiple of 8 and at least f3R = {self.f3r}, got {self.t5}")
        self.t_ld = self.t5 + self.f5r
        self.pk1, self.pk3r, self.pk5r, self.pkp = (PackedFilter(w, dtype) for w in (w1, w3r, w5r, wp))
        self.blob = None
        nbytes = _lib.load().tlxmi_inception_head_param_bytes(self.cin, self.f1, self.f3r, self.f5r, self.proj) if dtype == torch.float16 else 0
        if nbytes:
            self.blob = inception_head_pack(*(w.detach() for w in (w1, w3r, w5r, wp)))
            assert self.blob.numel() == nbytes


def _inception_head_desc(x, p, y_ld, t_ld):
    N, H, W, ld = x.shape
    return _lib.InceptionHeadDesc(dtype=dt_code(x.dtype), N=N, H=H, W=W, Cin=p.cin, f1=p.f1, f3R=p.f3r, f5R=p.f5r, proj=p.proj, x_ld=ld,
                                  y_ld=y_ld, t_ld=t_ld, y_proj_off=p.op, t_f5_off=p.t5)


def inception_head_takes(x, params, y_ld=None, t_ld=None):
    """Whether the library's tlxmi_inception_head takes this NHWC map with these parameters (fp16, the widths and pitches of
    include/tlxmi.h): what fused=True needs."""
    if x.dim() != 4 or x.dtype != torch.float16 or not x.is_contiguous() or params.blob is None:
        return False
    y_ld = params.cout if y_ld is None else int(y_ld)
    t_ld = params.t_ld if t_ld is None else int(t_ld)
    return bool(_lib.load().tlxmi_inception_head_supported(C.byref(_inception_head_desc(x, params, y_ld, t_ld))))


# (H, W, Cin, f1, f3R, f5R, proj) of the module heads where the one launch was measured FASTER than the layer-by-layer arm beyond the spread of
# both, at batch 256 on one MI355X (tools/googlenet_bench.py, profiles/googlenet/googlenet_bench_b256.txt): inception_head() keeps
# the launch there and runs the layers everywhere else by default.  MEASURED: it wins at `_ince3a` alone (0.59 of the layers' time: 13 n-tiles,
# one chunk at two workgroups a CU); `_ince3b` (0.96) and `_ince5a` (1.01) are inside the spread, the others take 1.06 - 1.15 (`_ince4a` .. `_ince4d`),
# 1.38 (`_ince5b`) and 1.58 (`_ince4e`) x the layers' time.  Shapes other than those nine are unmeasured and run layer by layer.
INCEPTION_HEAD_WINS = frozenset({(27, 27, 192, 64, 96, 16, 32)})


def _inception_head_routed(H, W, p):
    return (H, W, p.cin, p.f1, p.f3r, p.f5r, p.proj) in INCEPTION_HEAD_WINS


def inception_head_supported(x, params, y_ld=None, t_ld=None):
    """Whether inception_head() runs tlxmi_inception_head on this map by default: the "inception_head" option on, the measured table
    keeps the shape (INCEPTION_HEAD_WINS) and the library takes the call (inception_head_takes)."""
    return bool(_options["inception_head"] and x.dim() == 4 and _inception_head_routed(x.shape[1], x.shape[2], params)
                and inception_head_takes(x, params, y_ld, t_ld))


def inception_head(x, params, fused=None, out=None, mid=None):
    """Everything of an Inception module (googlenet.py:41-65) that reads its input, on an NHWC map x (N, H, W, x_ld) whose first
    Cin = params.cin channels are the input (the columns behind them are not read):
        y[..., :f1] = relu(x . W1),   t[..., :f3R] = x . W3r,   t[..., t5:t5 + f5R] = x . W5r   (the reduce convs are linear),
        y[..., op:op + proj] = relu(maxpool 3/1/1 (x) . Wp)        (positions outside the image take no part in the max)
    -> (y, t): y (N, H, W, params.cout) or `out`, t (N, H, W, params.t_ld) or `mid` (their last axes are the pitches, multiples of 8).
    The slices [f1, op) of y — the module's 3x3 and 5x5 convs write them from t — and every other column are left untouched.
    params: InceptionParams.  One launch (tlxmi_inception_head: x read once, the pooled map kept in LDS) when the "inception_head"
    option is on, the precision is fp16, the measured table keeps the shape and the library takes it (inception_head_supported);
    otherwise — and always for fp32 — tlxmi_conv2d three times into the slices, tlxmi_maxpool2d, tlxmi_conv2d.  fused=True / False
    forces one form (tests, tools/); True raises where the launch is not supported."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    p = params
    if x.dtype != p.dtype or ld < p.cin or ld % 8 or not x.is_contiguous():
        raise RuntimeError(f"inception_head: x must be a dense NHWC map of the parameters' dtype with at least {p.cin} channels at a pitch "
                           f"that is a multiple of 8, got {tuple(x.shape)} {x.dtype}")
    out, y_ld = _out_map("inception_head", out, N, H, W, p.cout, x.dtype, x.device, p.cout, multiple=8,
                         what=f"a dense ({N}, {H}, {W}, >= {p.cout}) map of x's dtype at a pitch that is a multiple of 8")
    mid, t_ld = _out_map("inception_head", mid, N, H, W, p.t_ld, x.dtype, x.device, p.t_ld, multiple=8,
                         what=f"(mid) a dense ({N}, {H}, {W}, >= {p.t_ld}) map of x's dtype at a pitch that is a multiple of 8")
    takes = lambda: inception_head_takes(x, p, y_ld, t_ld)      # noqa: E731
    # the option and the table first: the library's predicate is asked only where they keep the launch
    fused = _use_fused("inception_head", fused, takes, lambda: _options["inception_head"] and _inception_head_routed(H, W, p) and takes(),
                       lambda: f"{tuple(x.shape)} {x.dtype} with Cin {p.cin}, widths {p.f1} / {p.f3r} / {p.f5r} / {p.proj}, y_ld {y_ld}, t_ld {t_ld}")
    es = x.element_size()
    M = N * H * W
    if _sizing():
        _note_act(x.numel() * es, M * y_ld * es, M * t_ld * es)

    def launch():
        if fused:
            desc = _inception_head_desc(x, p, y_ld, t_ld)
            _lib.call("tlxmi_inception_head", C.byref(desc), _p(x), _p(p.blob), _p(out), _p(mid), _stream())
            return
        xin = x[..., :p.cin]
        conv2d(xin, p.pk1, act=ACT_RELU, out=out[..., :p.f1], out_ld=y_ld, x_ld=ld)
        conv2d(xin, p.pk3r, out=mid[..., :p.f3r], out_ld=t_ld, x_ld=ld)
        conv2d(xin, p.pk5r, out=mid[..., p.t5:p.t5 + p.f5r], out_ld=t_ld, x_ld=ld)
        pooled = torch.empty((N, H, W, p.cin), dtype=x.dtype, device=x.device)
        _lib.call("tlxmi_maxpool2d", _p(x), _p(pooled), dt_code(x.dtype), N, H, W, p.cin, ld, p.cin, 3, 3, 1, 1, 1, 1, H, W, _stream())
        conv2d(pooled, p.pkp, act=ACT_RELU, out=out[..., p.op:p.op + p.proj], out_ld=y_ld)
    nout = p.f1 + p.f3r + p.f5r + p.proj
    _timed(launch, lambda: ((M * (p.cin + nout) + p.cin * nout) * es, 2 * M * p.cin * nout,
                            (N, H, W, p.cin, nout, "inception_head" if fused else "conv-conv-conv-pool-conv")))      # the chain is one entry
    return out, mid


# ---------------------------------------------------------------------------------------------
# SqueezeNet's Fire module: squeeze 1x1 -> expand 1x1 | expand 3x3
# ---------------------------------------------------------------------------------------------
def fire_module_pack(ws, bs, w1, b1, w3, b3):
    """The parameter image tlxmi_fire_module reads (include/tlxmi.h), as one uint8 tensor on the operands' device: fp16 Ws [sq][CinP],
    W1 [E1P][K1P], W3 [E3P][K3P] with k = (3 r + s) sq + c, then fp32 bs [sq], b1 [E1P], b3 [E3P]; CinP, K1P, K3P = Cin, sq, 9 sq
    rounded up to 32, E1P, E3P = e1, e3 rounded up to 16, every pad zero.  ws (sq, Cin, 1, 1), w1 (e1, sq, 1, 1), w3 (e3, sq, 3, 3)."""
    sq, cin = int(ws.shape[0]), int(ws.shape[1])
    e1, e3 = int(w1.shape[0]), int(w3.shape[0])
    dev, h, f = ws.device, torch.float16, torch.float32
    e1p, e3p = _round_up(e1, 16), _round_up(e3, 16)
    return _param_image(_zero_padded(ws.reshape(sq, cin), (sq, _round_up(cin, 32)), h, dev),
                        _zero_padded(w1.reshape(e1, sq), (e1p, _round_up(sq, 32)), h, dev),
                        _zero_padded(w3.detach().permute(0, 2, 3, 1).reshape(e3, 9 * sq), (e3p, _round_up(9 * sq, 32)), h, dev),
                        _zero_padded(bs, (sq,), f, dev), _zero_padded(b1, (e1p,), f, dev), _zero_padded(b3, (e3p,), f, dev))


class FireParams:
    """The three convs of one Fire module in the forms both arms of fire_module() read: a PackedFilter and an fp32 bias each for the
    layer-by-layer arm, and — fp16, inside the library's ranges — the one-buffer image of tlxmi_fire_module (fire_module_pack).
    ws (sq, Cin, 1, 1), w1 (e1, sq, 1, 1), w3 (e3, sq, 3, 3) and their biases.  The output map's slices are [0, e1) | [e1, e1 + e3)
    = the concatenation of the reference (squeezenet.py:52).  Cin, sq and e1 must be multiples of 8 (the squeeze map feeds 16-byte
    vectors and the 3x3's slice must start on a 16-byte boundary): other widths are REFUSED here, in both arms.
    packed / biases: the layers' own (PackedFilter x 3) and (fp32 bias x 3) at this precision, where a model holds them already."""

    def __init__(self, ws, bs, w1, b1, w3, b3, dtype, packed=None, biases=None):
        self.sq, self.cin = int(ws.shape[0]), int(ws.shape[1])
        self.e1, self.e3 = int(w1.shape[0]), int(w3.shape[0])
        if (int(w1.shape[1]) != self.sq or int(w3.shape[1]) != self.sq or tuple(w3.shape[2:]) != (3, 3) or tuple(ws.shape[2:]) != (1, 1)
                or tuple(w1.shape[2:]) != (1, 1) or any(n <= 0 or n % 8 for n in (self.cin, self.sq, self.e1))):
            raise RuntimeError(f"FireParams: a 1x1 squeeze (sq, Cin), a 1x1 expand (e1, sq) and a 3x3 expand (e3, sq) are expected, Cin, sq and "
                               f"e1 multiples of 8; got {tuple(ws.shape)}, {tuple(w1.shape)}, {tuple(w3.shape)}")
        self.dtype, self.cout = dtype, self.e1 + self.e3
        self.pks, self.pk1, self.pk3 = packed if packed is not None else (PackedFilter(w, dtype) for w in (ws, w1, w3))
        self.bs, self.b1, self.b3 = biases if biases is not None else (_f32(b) for b in (bs, b1, b3))
        self.blob = None
        nbytes = _lib.load().tlxmi_fire_module_param_bytes(self.cin, self.sq, self.e1, self.e3) if dtype == torch.float16 else 0
        if nbytes:
            self.blob = fire_module_pack(*(t.detach() for t in (ws, bs, w1, b1, w3, b3)))
            assert self.blob.numel() == nbytes


def _fire_module_desc(x, p, y_ld):
    N, H, W, ld = x.shape
    return _lib.FireModuleDesc(dtype=dt_code(x.dtype), N=N, H=H, W=W, Cin=p.cin, sq=p.sq, e1=p.e1, e3=p.e3, x_ld=ld, y_ld=y_ld)


def fire_module_takes(x, params, y_ld=None):
    """Whether the library's tlxmi_fire_module takes this NHWC map with these parameters (fp16, the widths and pitches of
    include/tlxmi.h): what fused=True needs."""
    if x.dim() != 4 or x.dtype != torch.float16 or not x.is_contiguous() or params.blob is None:
        return False
    y_ld = params.cout if y_ld is None else int(y_ld)
    return bool(_lib.load().tlxmi_fire_module_supported(C.byref(_fire_module_desc(x, params, y_ld))))


# (H, W, Cin, sq, e1, e3) of the modules where the one launch was measured FASTER than the layer-by-layer arm beyond the spread of both — its
# slowest round against the layers' fastest — at batch 256 on one MI355X (tools/squeezenet_bench.py,
# profiles/squeezenet/squeezenet_bench_b256.txt): fire_module() keeps the launch there and runs the layers everywhere else by
# default.  MEASURED over the twelve distinct shapes of both versions: it wins the three sq = 32 modules at 26 x 26 / 27 x 27 (0.83 - 0.93 of
# the layers' time); it takes 1.07 - 1.20 x the layers' time at the 54 x 54 / 55 x 55 modules and at sq = 48, 1.24 - 1.40 x at sq = 64.
# Shapes other than those twelve are unmeasured and run layer by layer.
FIRE_MODULE_WINS = frozenset({(26, 26, 256, 32, 128, 128), (27, 27, 128, 32, 128, 128), (27, 27, 256, 32, 128, 128)})


def _fire_module_routed(H, W, p):
    return (H, W, p.cin, p.sq, p.e1, p.e3) in FIRE_MODULE_WINS


def fire_module_supported(x, params, y_ld=None):
    """Whether fire_module() runs tlxmi_fire_module on this map by default: the "fire_module" option on, the measured table keeps the
    shape (FIRE_MODULE_WINS) and the library takes the call (fire_module_takes)."""
    return bool(_options["fire_module"] and x.dim() == 4 and _fire_module_routed(x.shape[1], x.shape[2], params)
                and fire_module_takes(x, params, y_ld))


def fire_module(x, params, fused=None, out=None):
    """A Fire module (squeezenet.py:37-52) on an NHWC map x (N, H, W, x_ld) whose first Cin = params.cin channels are the input (the
    columns behind them are not read):
        s = relu(x . Ws + bs),   y[..., :e1] = relu(s . W1 + b1),   y[..., e1:e1 + e3] = relu(conv3x3 pad 1 (s) . W3 + b3)
    -> y (N, H, W, e1 + e3), or written into `out` (its last axis is the pitch, a multiple of 8; nothing behind e1 + e3 is written).
    params: FireParams.  One launch (tlxmi_fire_module: x read once, the squeeze map kept in LDS) when the "fire_module" option is
    on, the precision is fp16, the measured table keeps the shape and the library takes it (fire_module_supported); otherwise — and
    always for fp32 — tlxmi_conv2d three times with bias + ReLU epilogues, the two expands into their slices.  fused=True / False
    forces one form (tests, tools/); True raises where the launch is not supported."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    p = params
    if x.dtype != p.dtype or ld < p.cin or ld % 8 or not x.is_contiguous():
        raise RuntimeError(f"fire_module: x must be a dense NHWC map of the parameters' dtype with at least {p.cin} channels at a pitch "
                           f"that is a multiple of 8, got {tuple(x.shape)} {x.dtype}")
    out, y_ld = _out_map("fire_module", out, N, H, W, p.cout, x.dtype, x.device, p.cout, multiple=8,
                         what=f"a dense ({N}, {H}, {W}, >= {p.cout}) map of x's dtype at a pitch that is a multiple of 8")
    takes = lambda: fire_module_takes(x, p, y_ld)      # noqa: E731
    # the option and the table first: the library's predicate is asked only where they keep the launch
    fused = _use_fused("fire_module", fused, takes, lambda: _options["fire_module"] and _fire_module_routed(H, W, p) and takes(),
                       lambda: f"{tuple(x.shape)} {x.dtype} with Cin {p.cin}, sq {p.sq}, e1 {p.e1}, e3 {p.e3}, y_ld {y_ld}")
    es = x.element_size()
    M = N * H * W
    if _sizing():
        _note_act(x.numel() * es, M * y_ld * es)

    def launch():
        if fused:
            desc = _fire_module_desc(x, p, y_ld)
            _lib.call("tlxmi_fire_module", C.byref(desc), _p(x), _p(p.blob), _p(out), _stream())
            return
        s = conv2d(x[..., :p.cin], p.pks, shift=p.bs, act=ACT_RELU, x_ld=ld)
        conv2d(s, p.pk1, shift=p.b1, act=ACT_RELU, out=out[..., :p.e1], out_ld=y_ld)
        conv2d(s, p.pk3, 1, 1, 1, shift=p.b3, act=ACT_RELU, out=out[..., p.e1:p.cout], out_ld=y_ld)
    nw = p.cin * p.sq + p.sq * p.e1 + 9 * p.sq * p.e3
    _timed(launch, lambda: ((M * (p.cin + p.cout) + nw) * es, 2 * M * nw,
                            (N, H, W, p.cin, p.cout, "fire_module" if fused else "conv-conv-conv")))      # the chain is one entry
    return out


# ---------------------------------------------------------------------------------------------
# DPN's dual-path 1x1 conv: split -> add onto the residual path | concat onto the dense path
# ---------------------------------------------------------------------------------------------
class DualPathParams:
    """The `c` conv of a DualPathFactory (dpn.py:103-105) in the forms both arms of dual_path_conv1x1() read: the whole (bw + inc, K, 1, 1)
    filter packed once for the launch, and its row ranges [0, bw) — the residual path — and [bw, bw + inc) — the dense path — packed once
    each for the layer-by-layer arm.  w: the filter as the kernels see it, i.e. with the host's zero padding already in (K, bw and inc
    multiples of 8: a DPN width that is not is padded by the model, never refused here and never seen by a kernel).
    packed: the layer's own PackedFilter of w at this precision, where a model holds it already."""

    def __init__(self, w, bw, dtype, packed=None):
        cout, self.K = int(w.shape[0]), int(w.shape[1])
        self.bw, self.inc = int(bw), cout - int(bw)
        if tuple(w.shape[2:]) != (1, 1) or any(n <= 0 or n % 8 for n in (self.K, self.bw, self.inc)):
            raise RuntimeError(f"DualPathParams: a 1x1 filter (bw + inc, K) with K, bw and inc positive multiples of 8 is expected; got "
                               f"{tuple(w.shape)} with bw {bw}")
        self.dtype = dtype
        w = w.detach()
        self.pk = packed if packed is not None else PackedFilter(w, dtype)
        self.pk_res, self.pk_dense = PackedFilter(w[:self.bw], dtype), PackedFilter(w[self.bw:], dtype)


def dual_path_takes(t, params, state, dense_off):
    """Whether the library's tlxmi_dual_path_conv1x1 takes these operands (fp16, the widths and pitches of include/tlxmi.h): what
    fused=True needs."""
    if t.dtype != torch.float16 or state.dtype != torch.float16 or params.dtype != torch.float16:
        return False
    rows = state.numel() // state.shape[-1]
    return bool(_lib.load().tlxmi_dual_path_conv1x1_supported(F16, rows, params.K, params.bw, params.inc, int(dense_off), t.shape[-1],
                                                               state.shape[-1]))


# (pixels per image H * W, K, bw, inc) of the `c` convs where the one launch was measured FASTER than the two layered launches in every
# round — its slowest round against the layers' fastest — at batch 256 on one MI355X (tools/dpn_bench.py,
# profiles/dpn/dpn_bench_b256.txt): dual_path_conv1x1() keeps the launch there and runs the layers everywhere else by
# default.  dense_off is not part of the key: it moves a store, not the work (each shape was timed at its stage's last block).
# MEASURED over the eight distinct shapes of DPN-68 and DPN-107 at 224 x 224: the launch wins all four of DPN-68 (0.66 - 0.82 of the
# layers' time) and DPN-107's 56 x 56 and 28 x 28 stages (0.70, 0.83); at DPN-107's 14 x 14 (K 800, bw 1024) and 7 x 7 (K 1600, bw 2048)
# stages it is 0.99 / 1.00 of the layers' time with overlapping rounds — not a win, so they stay on the layers.  Shapes other than
# those eight (DPN-92 / 98 / 131, other input sizes) are unmeasured and run layer by layer.
DUAL_PATH_WINS = frozenset({(3136, 128, 64, 16), (784, 256, 128, 32), (196, 512, 256, 32), (49, 1024, 512, 64),
                            (3136, 200, 256, 24), (784, 400, 512, 64)})


def _dual_path_routed(pixels, p):
    return (pixels, p.K, p.bw, p.inc) in DUAL_PATH_WINS


def dual_path_conv1x1(t, pk, state, bw, dense_off, fused=None):
    """The conv that ends a DualPathFactory (dpn.py:121-126), IN PLACE on the stage buffer `state` (N, H, W, ld):
        state[..., :bw] += t . W[:bw]          (the residual path: fp32 add, one rounding)
        state[..., dense_off:dense_off + inc] = t . W[bw:]          (the dense path: this block's inc new channels)
    t (N, H, W, t_ld) NHWC, its first K channels the operand — already activated: the 3x3's epilogue applied this conv's BatchNorm +
    ReLU.  pk: DualPathParams (bw must be its bw).  Nothing else of state is written; the columns [bw, dense_off) are the earlier
    blocks' dense channels.  One launch (tlxmi_dual_path_conv1x1) when the "dual_path" option is on, the precision is fp16, the measured
    table keeps the shape and the library takes it; otherwise — and always for fp32: the parity reference — tlxmi_conv2d twice on the
    same packed operands: filter rows [0, bw) with res = out = state, rows [bw, bw + inc) into the column slice at dense_off.
    fused=True / False forces one form (tests, tools/); True raises where the launch is not supported.  -> state."""
    need_gpu(t, "input")
    p = pk
    if t.dim() == 2:
        t = t.view(t.shape[0], 1, 1, t.shape[1])
    if state.dim() == 2:
        state = state.view(state.shape[0], 1, 1, state.shape[1])
    N, H, W, ld = state.shape
    t_ld, dense_off = t.shape[-1], int(dense_off)
    vw = vec(t.dtype)
    if (int(bw) != p.bw or t.dtype != p.dtype or state.dtype != p.dtype or tuple(t.shape[:3]) != (N, H, W) or t_ld < p.K or t_ld % vw
            or ld % vw or dense_off % vw or dense_off < p.bw or dense_off + p.inc > ld or not t.is_contiguous() or not state.is_contiguous()):
        raise RuntimeError(f"dual_path_conv1x1: t {tuple(t.shape)} {t.dtype} and state {tuple(state.shape)} {state.dtype} must be dense NHWC maps "
                           f"of the parameters' dtype over the same pixels, t with at least K = {p.K} channels, bw = {p.bw} <= dense_off = "
                           f"{dense_off} and dense_off + inc = {dense_off + p.inc} <= the state's pitch, pitches and dense_off multiples of {vw}")
    takes = lambda: dual_path_takes(t, p, state, dense_off)      # noqa: E731
    # the option and the table first: the library's predicate is asked only where they keep the launch
    fused = _use_fused("dual_path_conv1x1", fused, takes, lambda: _options["dual_path"] and _dual_path_routed(H * W, p) and takes(),
                       lambda: f"t {tuple(t.shape)} {t.dtype}, state {tuple(state.shape)} with K {p.K}, bw {p.bw}, inc {p.inc}, dense_off {dense_off}")
    es = t.element_size()
    M = N * H * W
    if _sizing():
        _note_act(t.numel() * es, M * ld * es)
    if not fused:       # two launches, each its own probe entry
        conv2d(t, p.pk_res, res=state, out=state, out_ld=ld, res_ld=ld)
        conv2d(t, p.pk_dense, out=state[..., dense_off:dense_off + p.inc], out_ld=ld)
        return state
    args = (F16, M, p.K, p.bw, p.inc, dense_off, t_ld, ld, _p(t), _p(p.pk.buf), _p(state), _stream())
    _timed(lambda: _lib.call("tlxmi_dual_path_conv1x1", *args),
           lambda: ((M * (p.K + 2 * p.bw + p.inc) + (p.bw + p.inc) * p.K) * es, 2 * M * (p.bw + p.inc) * p.K,
                    (N, H, W, p.K, p.bw, p.inc, "dual_path")))
    return state


# ---------------------------------------------------------------------------------------------
# HarDNet's linked conv: a layer that convolves the concat of up to 8 column slices of the block buffer
# ---------------------------------------------------------------------------------------------
class LinkConvParams:
    """A multi-link layer of a HarDBlock (hardnet.py:85-97) in the form both arms of link_conv2d() read: the (Cout, K, R, R) filter
    packed once — K the sum of the links' widths in link order — with the epilogue's fp32 scale and shift.  w, scale, shift: as the
    kernels see them, i.e. with the host's zero padding already in (Cout and every link width multiples of 8: a HarDNet width that is
    not is padded by the model, never refused here and never seen by a kernel).  packed: the layer's own PackedFilter of w at this
    precision, where a model holds it already."""

    def __init__(self, w, scale, shift, dtype, packed=None):
        self.Cout, self.K, self.R, s_ = (int(v) for v in w.shape)
        if self.R != s_ or self.R not in (1, 3) or self.Cout % 8 or self.K % 8:
            raise RuntimeError(f"LinkConvParams: a (Cout, K, R, R) filter with R 1 or 3 and Cout, K multiples of 8 is expected; got {tuple(w.shape)}")
        self.dtype = dtype
        self.pk = packed if packed is not None else PackedFilter(w.detach(), dtype)
        self.scale, self.shift = _f32(scale), _f32(shift)


def _link_conv_desc(buf, segments, p, act, out, out_ld):
    N, H, W, ld = buf.shape
    es = buf.element_size()
    d = out.data_ptr() - buf.data_ptr()
    inside = 0 <= d < buf.numel() * es          # out is a view into the map: its column (anything but a slice of pixel 0 is refused)
    return _lib.LinkConvDesc(dtype=dt_code(buf.dtype), N=N, H=H, W=W, R=p.R, nseg=len(segments),
                             seg_off=(C.c_int32 * 8)(*[int(o) for o, _ in segments]), seg_c=(C.c_int32 * 8)(*[int(c) for _, c in segments]),
                             Cout=p.Cout, x_ld=ld, y_ld=int(out_ld), y_off=d // es if inside else -1, act=int(act))


def link_conv_takes(buf, segments, params, act, out, out_ld):
    """Whether the library's tlxmi_link_conv2d takes these operands (fp16, the widths, pitches and disjointness of include/tlxmi.h): what
    fused=True needs."""
    if buf.dtype != torch.float16 or out.dtype != torch.float16 or params.dtype != torch.float16 or not 1 <= len(segments) <= 8:
        return False
    return bool(_lib.load().tlxmi_link_conv2d_supported(C.byref(_link_conv_desc(buf, segments, params, act, out, out_ld))))


# (pixels per image H * W, R, the links' widths in link order, Cout) of the multi-link layers where the one launch was measured FASTER
# than the layered arm in every round — its slowest round against the layers' fastest — at batch 256 on one MI355X
# (tools/hardnet_bench.py, profiles/hardnet/hardnet_bench_b256.txt): link_conv2d() keeps the launch there and runs the
# layers everywhere else, unmeasured shapes included, by default.  Where the slices sit is not part of the key: it moves addresses, not
# the work.
# MEASURED over the 49 distinct multi-link shapes of HarDNet-85 (34, all 3x3) and HarDNet-39ds (15, all 1x1) at 224 x 224: the launch wins
# every 1x1 shape (0.39 - 0.73 of the layers' time: there the copy moves more bytes than the conv) and two small 3x3 shapes at 14 x 14
# (0.86, 0.97); at the other 32 3x3 shapes the tuned tlxmi_conv2d behind its copies is FASTER (the launch takes 1.02 - 1.58 of its time),
# so they stay on the layers.  Shapes other than those 49 (HarDNet-68 / 68ds, other input sizes) are unmeasured and run layer by layer.
LINK_CONV_WINS = frozenset({
    (3136, 1, (16, 48), 32), (3136, 1, (16, 32, 48), 40),
    (784, 1, (24, 96), 32), (784, 1, (24, 32, 96), 56), (784, 1, (24, 56), 32), (784, 1, (24, 32, 56, 96), 88), (784, 1, (24, 88), 32),
    (784, 1, (24, 32, 88), 56), (784, 1, (24, 32, 56, 88, 96), 136),
    (196, 1, (64, 320), 104), (196, 1, (64, 104, 320), 168), (196, 1, (64, 168), 104), (196, 1, (64, 104, 168, 320), 264),
    (49, 1, (160, 640), 256), (49, 1, (160, 256, 640), 416),
    (196, 3, (40, 104), 64), (196, 3, (40, 176), 64)})


def _link_conv_routed(pixels, segments, p):
    return (pixels, p.R, tuple(int(c) for _, c in segments), p.Cout) in LINK_CONV_WINS


def link_conv2d(buf, segments, params, act, out, out_ld=None, fused=None):
    """A multi-link layer of a HarDBlock on the block buffer `buf` (N, H, W, ld) NHWC:
        out[..., :Cout] = act(scale * conv RxR pad R/2 (concat_s buf[..., off_s:off_s + c_s]) + shift)
    segments: [(off, c)] in link order (need not ascend), every value a multiple of 8.  params: LinkConvParams.  out: a column slice of
    buf that overlaps no segment (a view), or a map of its own; out_ld its pixel pitch (default: out's pixel stride).
    One launch (tlxmi_link_conv2d) when the "link_conv" option is on, the precision is fp16, the measured table keeps the shape and the
    library takes it; otherwise — and always for fp32: the parity reference — one tlxmi_copy_channels a segment into a scratch map,
    then tlxmi_conv2d on the same packed filter.  fused=True / False forces one form (tests, tools/); True raises where the launch is
    not supported.  -> out."""
    need_gpu(buf, "input")
    p = params
    N, H, W, ld = buf.shape
    segments = [(int(o), int(c)) for o, c in segments]
    vw = vec(buf.dtype)
    out_ld = int(out_ld if out_ld is not None else out.stride(2))
    if (buf.dtype != p.dtype or out.dtype != p.dtype or not buf.is_contiguous() or tuple(out.shape[:3]) != (N, H, W) or out.shape[-1] < p.Cout
            or not segments or sum(c for _, c in segments) != p.K or ld % vw or out_ld % vw
            or any(o < 0 or c <= 0 or o % vw or c % vw or o + c > ld for o, c in segments)):
        raise RuntimeError(f"link_conv2d: buf {tuple(buf.shape)} {buf.dtype} must be a dense NHWC map of the parameters' dtype, out "
                           f"{tuple(out.shape)} a map over the same pixels with at least Cout = {p.Cout} channels, the segments {segments} "
                           f"column slices of buf whose widths add up to K = {p.K}, every offset, width and pitch a multiple of {vw}")
    takes = lambda: link_conv_takes(buf, segments, p, act, out, out_ld)      # noqa: E731
    # the option and the table first: the library's predicate is asked only where they keep the launch
    fused = _use_fused("link_conv2d", fused, takes, lambda: _options["link_conv"] and _link_conv_routed(H * W, segments, p) and takes(),
                       lambda: f"buf {tuple(buf.shape)} {buf.dtype} with segments {segments}, R {p.R}, Cout {p.Cout}, act {act}, out at pitch {out_ld}")
    es = buf.element_size()
    M = N * H * W
    if _sizing():
        _note_act(buf.numel() * es, M * out_ld * es)

    def launch():
        if fused:
            _lib.call("tlxmi_link_conv2d", C.byref(_link_conv_desc(buf, segments, p, act, out, out_ld)), _p(buf), _p(p.pk.buf), _p(p.scale),
                      _p(p.shift), _p(out), _stream())
            return
        gathered = torch.empty((N, H, W, p.K), dtype=buf.dtype, device=buf.device)
        k = 0
        for o, c in segments:
            copy_channels_into(buf[..., o:o + c], gathered, k, x_ld=ld)
            k += c
        conv2d(gathered, p.pk, 1, p.R // 2, 1, p.scale, p.shift, act=act, out=out, out_ld=out_ld)
    _timed(launch, lambda: ((M * (p.K + p.Cout) + p.Cout * p.K * p.R * p.R) * es, 2 * M * p.Cout * p.K * p.R * p.R,
                            (N, H, W, p.K, p.Cout, p.R, "link_conv" if fused else "copy-conv")))      # the chain is one entry
    return out


# ---------------------------------------------------------------------------------------------
# ReXNet's gated projection: SE gate -> ReLU6 -> 1x1 conv + BN -> shortcut onto a channel prefix
# ---------------------------------------------------------------------------------------------
def _gated_conv_desc(x, gate, pk, res, res_c, pre_act, out_ld):
    """The positional geometry of tlxmi_gated_conv1x1 / _supported: (dtype, rows, HW, K, Cout, x_ld, gate_ld, y_ld, res_ld, res_c)."""
    N, H, W, ld = x.shape
    return (dt_code(x.dtype), N * H * W, H * W, pk.Cin, pk.Cout, ld, 0 if gate is None else gate.shape[-1], int(out_ld),
            res.shape[-1] if res_c else 0, int(res_c))


def gated_conv1x1_takes(x, gate, pk, res=None, res_c=0, pre_act=ACT_RELU6, out_ld=None):
    """Whether the library's tlxmi_gated_conv1x1 takes these operands (fp16, the widths and pitches of include/tlxmi.h): what
    fused=True needs."""
    if x.dtype != torch.float16 or pk.dtype != torch.float16 or pk.R != 1 or pk.S != 1 or x.dim() != 4:
        return False
    d = _gated_conv_desc(x, gate, pk, res, res_c, pre_act, pk.Cout if out_ld is None else out_ld)
    return bool(_lib.load().tlxmi_gated_conv1x1_supported(*d, int(pre_act)))


# (pixels per image H * W, K, Cout, res_c, gated) — K and Cout as the kernel sees them, padded to 8; res_c the true shortcut width — of
# the projections where the one launch was measured FASTER than the layered arm on every alternation at batch 256 on one MI355X
# (tools/rexnet_bench.py, profiles/rexnet/): gated_conv1x1() keeps the launch there and runs the layers everywhere else,
# unmeasured shapes included, by default.
# MEASURED over the 32 distinct projections of ReXNet-1.0 and ReXNet-2.0 at 224 x 224: the launch wins ALL of them, at 0.26 - 0.84 of the
# layered arm's time (0.26 - 0.59 at 112 x 112 .. 14 x 14, 0.60 - 0.84 at 7 x 7, where K reaches 2088 and the A tile is re-read by up to six
# column tiles); both arms give identical bits at every shape.  Shapes other than those 32 (ReXNet-1.3 / 1.5 / 3.0, other input sizes) are
# unmeasured and run layer by layer.
GATED_CONV_WINS = frozenset({
    (12544, 32, 16, 0, False), (3136, 96, 32, 0, False), (3136, 168, 40, 27, False), (784, 232, 56, 0, True), (784, 304, 64, 50, True),
    (196, 368, 72, 0, True), (196, 432, 88, 72, True), (196, 504, 96, 84, True), (196, 576, 112, 95, True), (196, 640, 120, 106, True),
    (196, 704, 128, 117, True), (49, 768, 144, 0, True), (49, 840, 152, 140, True), (49, 912, 168, 151, True), (49, 976, 176, 162, True),
    (49, 1048, 192, 174, True),
    (12544, 64, 32, 0, False), (3136, 192, 56, 0, False), (3136, 328, 80, 54, False), (784, 464, 104, 0, True), (784, 600, 128, 100, True),
    (196, 736, 144, 0, True), (196, 864, 168, 144, True), (196, 1008, 192, 167, True), (196, 1144, 216, 190, True), (196, 1272, 240, 212, True),
    (196, 1408, 264, 234, True), (49, 1544, 280, 0, True), (49, 1680, 304, 280, True), (49, 1816, 328, 302, True), (49, 1944, 352, 324, True),
    (49, 2088, 376, 347, True)})


def _gated_conv_routed(pixels, pk, res_c, gated):
    return (pixels, pk.Cin, pk.Cout, int(res_c), bool(gated)) in GATED_CONV_WINS


def gated_conv1x1_supported(x, gate, pk, res=None, res_c=0, pre_act=ACT_RELU6, out_ld=None):
    """Whether gated_conv1x1() runs tlxmi_gated_conv1x1 on these operands by default: the "gated_conv" option on, the shape in the
    measured table and the library's predicate."""
    return bool(_options["gated_conv"] and _gated_conv_routed(x.shape[1] * x.shape[2], pk, res_c, gate is not None)
                and gated_conv1x1_takes(x, gate, pk, res, res_c, pre_act, out_ld))


def gated_conv1x1(x, gate, pk, scale, shift, res=None, res_c=0, pre_act=ACT_RELU6, out=None, out_ld=None, fused=None):
    """The tail of ReXNet's LinearBottleneck (rexnet.py:61-64, :84-95) on an NHWC map x (N, H, W, x_ld) whose first K = pk.Cin channels
    are the operand:
        y[..., n] = conv1x1(pre_act(x[..., :K] * gate[image, :K]))[n] * scale[n] + shift[n] + (res[..., n] if n < res_c else 0)
    gate: (N, gate_ld >= K) in x's dtype, or None (no gate); pre_act: ACT_RELU6 or ACT_NONE; pk: the PackedFilter of the (Cout, K, 1, 1)
    filter; scale / shift: fp32 [Cout]; res: a dense NHWC map over the same pixels whose first res_c channels are added — res_c any
    integer 0 .. Cout; what res holds behind them is never used.  -> y (N, H, W, Cout), or written into `out` (a dense map whose last
    axis is the pitch; with out_ld, a column slice of a wider buffer at that pitch); nothing behind Cout is written.
    One launch (tlxmi_gated_conv1x1) when the "gated_conv" option is on, the precision is fp16, the measured table keeps the shape and
    the library takes it; otherwise — and always for fp32: the parity reference — tlxmi_scale_channels -> tlxmi_affine_act (the ReLU6)
    -> tlxmi_conv2d with the shortcut as its residual: res itself where res_c == Cout, else a zero-filled Cout-wide copy of its first
    res_c columns (tlxmi_copy_channels; a dense copy where res_c is no whole 16-byte chunk).  fused=True / False forces one form
    (tests, tools/); True raises where the launch is not supported."""
    need_gpu(x, "input")
    if x.dim() != 4:
        raise RuntimeError(f"gated_conv1x1: x must be an NHWC map, got {tuple(x.shape)}")
    N, H, W, ld = x.shape
    K, Cout, v = pk.Cin, pk.Cout, vec(x.dtype)
    res_c = int(res_c)
    if pk.R != 1 or pk.S != 1 or x.dtype != pk.dtype or ld < K or not x.is_contiguous() or K % v or ld % v or Cout % v:
        raise RuntimeError(f"gated_conv1x1: x must be a dense NHWC map of the filter's dtype with at least K = {K} channels, K, Cout = {Cout} "
                           f"and the pitch multiples of {v}, and the filter 1x1; got {tuple(x.shape)} {x.dtype} for a {pk.R}x{pk.S} filter")
    if gate is not None and (gate.dtype != x.dtype or gate.dim() != 2 or gate.shape[0] != N or gate.shape[1] < K or gate.shape[1] % v
                             or not gate.is_contiguous()):
        raise RuntimeError(f"gated_conv1x1: gate must be a dense ({N}, >= {K}) matrix of x's dtype at a pitch that is a multiple of {v}, "
                           f"got {tuple(gate.shape)} {gate.dtype}")
    if pre_act not in (ACT_NONE, ACT_RELU6):
        raise RuntimeError(f"gated_conv1x1: pre_act must be ACT_NONE or ACT_RELU6, got {pre_act}")
    if not 0 <= res_c <= Cout or (res_c and (res is None or res.dtype != x.dtype or tuple(res.shape[:3]) != (N, H, W) or res.shape[-1] < res_c
                                             or res.shape[-1] % v or not res.is_contiguous())):
        raise RuntimeError(f"gated_conv1x1: res_c = {res_c} must lie in 0 .. Cout = {Cout} and res be a dense ({N}, {H}, {W}, >= res_c) map of "
                           f"x's dtype at a pitch that is a multiple of {v}; got {None if res is None else tuple(res.shape)}")
    if out is None or out_ld is None:
        out, out_ld = _out_map("gated_conv1x1", out, N, H, W, Cout, x.dtype, x.device, Cout, multiple=v,
                               what=f"a dense ({N}, {H}, {W}, >= {Cout}) map of x's dtype whose pitch is a multiple of {v}")
    else:
        out_ld = int(out_ld)
        if out.dtype != x.dtype or tuple(out.shape[:3]) != (N, H, W) or out.shape[-1] < Cout or out_ld < Cout or out_ld % v:
            raise RuntimeError(f"gated_conv1x1: out must be a column slice of at least {Cout} channels over the same pixels at a pitch that is "
                               f"a multiple of {v}, got {tuple(out.shape)} at pitch {out_ld}")
    takes = lambda: gated_conv1x1_takes(x, gate, pk, res, res_c, pre_act, out_ld)      # noqa: E731
    # the option and the table first: the library's predicate is asked only where they keep the launch
    fused = _use_fused("gated_conv1x1", fused, takes,
                       lambda: _options["gated_conv"] and _gated_conv_routed(H * W, pk, res_c, gate is not None) and takes(),
                       lambda: f"x {tuple(x.shape)} {x.dtype}, gate {None if gate is None else tuple(gate.shape)}, K {K}, Cout {Cout}, "
                               f"res_c {res_c}, pre_act {pre_act}, out at pitch {out_ld}")
    es = x.element_size()
    M = N * H * W
    if _sizing():
        _note_act(x.numel() * es, M * out_ld * es, res.numel() * es if res_c else 0)

    def launch():
        if fused:
            d = _gated_conv_desc(x, gate, pk, res, res_c, pre_act, out_ld)
            _lib.call("tlxmi_gated_conv1x1", *d, _p(x), _p(gate), int(pre_act), _p(pk.buf), _p(scale), _p(shift), _p(res if res_c else None),
                      _p(out), _stream())
            return
        dt = dt_code(x.dtype)
        t, t_ld = x, ld
        if gate is not None:
            g = torch.empty((N, H, W, K), dtype=x.dtype, device=x.device)
            _lib.call("tlxmi_scale_channels", _p(t), _p(gate), _p(g), dt, N, H * W, K, t_ld, gate.shape[-1], K, _stream())
            t, t_ld = g, K
        if pre_act == ACT_RELU6:
            a = torch.empty((N, H, W, K), dtype=x.dtype, device=x.device)
            _lib.call("tlxmi_affine_act", _p(t), None, None, None, _p(a), dt, M, K, t_ld, 0, K, ACT_RELU6, 0.0, 0, _stream())
            t, t_ld = a, K
        r = None
        if res_c == Cout:
            r = res
        elif res_c:
            r = torch.zeros((N, H, W, Cout), dtype=x.dtype, device=x.device)
            if res_c % v == 0:
                copy_channels_into(res[..., :res_c], r, 0, x_ld=res.shape[-1])
            else:       # the shortcut ends inside a 16-byte chunk: a dense copy
                r[..., :res_c] = res[..., :res_c]
        conv2d(t if t_ld == K else t[..., :K], pk, 1, 0, 1, scale, shift, res=r, out=out, out_ld=out_ld, x_ld=None if t_ld == K else t_ld)
    _timed(launch, lambda: ((M * (K + Cout + res_c) + Cout * K) * es, 2 * M * Cout * K,
                            (N, H, W, K, Cout, "gated_conv" if fused else "gate-act-conv")))      # the chain is one entry
    return out


# ---------------------------------------------------------------------------------------------
# pooling / elementwise / norm
# ---------------------------------------------------------------------------------------------
def maxpool2d(x, kernel, stride, padding, out=None, out_ld=None):
    """nn.MaxPool2d on an NHWC map -> (N, Ho, Wo, C), or written into `out` (a column slice of a wider buffer, pixel pitch out_ld)."""
    need_gpu(x, "input")
    N, H, W, Cc = x.shape
    R, S = _pair(kernel)
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    Ho = (H + 2 * ph - R) // sh + 1
    Wo = (W + 2 * pw - S) // sw + 1
    y = out if out is not None else torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    y_ld = Cc if out is None else (out_ld if out_ld is not None else out.shape[-1])
    _lib.call("tlxmi_maxpool2d", _p(x), _p(y), dt_code(x.dtype), N, H, W, Cc, Cc, y_ld, R, S, sh, sw, ph, pw, Ho, Wo,
              _stream())
    return y


def avgpool2d(x, kernel, stride, padding, out=None, out_ld=None):
    """nn.AvgPool2d on an NHWC map; zero padding counts in the divisor.  `out` / out_ld as maxpool2d."""
    need_gpu(x, "input")
    N, H, W, Cc = x.shape
    R, S = _pair(kernel)
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    Ho = (H + 2 * ph - R) // sh + 1
    Wo = (W + 2 * pw - S) // sw + 1
    y = out if out is not None else torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    y_ld = Cc if out is None else (out_ld if out_ld is not None else out.shape[-1])
    _lib.call("tlxmi_avgpool2d", _p(x), _p(y), dt_code(x.dtype), N, H, W, Cc, Cc, y_ld, R, S, sh, sw, ph, pw, Ho, Wo, _stream())
    return y


def radix_gap(x, radix):
    """(N,H,W,radix*C) -> (N,C): mean over pixels of the sum of the radix splits (resnest.py:150-155)."""
    need_gpu(x, "input")
    N, H, W, RC = x.shape
    Cc = RC // radix
    g = torch.empty((N, Cc), dtype=x.dtype, device=x.device)
    _lib.call("tlxmi_radix_gap", _p(x), _p(g), dt_code(x.dtype), N, H * W, Cc, radix, RC, Cc, _stream())
    return g


def split_attention(x, logit, radix, cardinality):
    """x (N,H,W,radix*C), logit (N,radix*C) -> (N,H,W,C): rSoftmax over the radix axis (sigmoid for radix 1) and the
    weighted sum of the splits (resnest.py:53-82, 158-165)."""
    need_gpu(x, "input")
    N, H, W, RC = x.shape
    Cc = RC // radix
    y = torch.empty((N, H, W, Cc), dtype=x.dtype, device=x.device)
    ws = torch.empty((N, RC), dtype=torch.float32, device=x.device)      # attention weights, split order
    _lib.call("tlxmi_split_attention", _p(x), _p(logit), _p(ws), _p(y), dt_code(x.dtype), N, H * W, Cc, radix, cardinality,
              RC, logit.shape[-1], Cc, _stream())
    return y


def global_avgpool(x):
    """(N,H,W,C) or (N,L,C) -> (N,C) mean over the middle axes."""
    need_gpu(x, "input")
    N, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * Cc)
    y = torch.empty((N, Cc), dtype=x.dtype, device=x.device)
    _lib.call("tlxmi_global_avgpool", _p(x), _p(y), dt_code(x.dtype), N, HW, Cc, Cc, Cc, _stream())
    return y


def affine_act(x, scale=None, shift=None, res=None, act=ACT_NONE, act_param=0.0, res_after_act=False, out=None, out_ld=None):
    """y = act(x*scale[c] + shift[c] (+res)) over the last axis.  out_ld: the rows of `out` sit this many elements apart (a wider or
    pre-offset buffer)."""
    need_gpu(x, "input")
    if not x.is_contiguous():
        x = x.contiguous()
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = out if out is not None else torch.empty_like(x)
    if res is not None and not res.is_contiguous():
        res = res.contiguous()
    _lib.call("tlxmi_affine_act", _p(x), _p(scale), _p(shift), _p(res), _p(y), dt_code(x.dtype), rows, Cc, Cc,
              Cc if res is not None else 0, Cc if out_ld is None else int(out_ld), act, float(act_param),
              EPI_RES_AFTER_ACT if res_after_act else 0, _stream())
    return y


def act_flat(x, act, act_param=0.0):
    """Elementwise activation of a tensor of ANY shape: runs over the flat storage, so the channel count need not be a
    multiple of the 16-byte vector width and the memory layout (contiguous / channels_last) is kept.  A buffer whose
    element count is not a whole number of chunks (or that is not dense) takes one padded copy."""
    need_gpu(x, "input")
    if x.dtype != _precision:
        x = x.to(_precision)
    v = vec(x.dtype)
    dense = x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last))
    if not dense:
        x = x.contiguous()
    n = x.numel()
    if n == 0:
        return x.clone()
    if n % v == 0 and x.data_ptr() % 16 == 0:
        y = torch.empty_like(x)          # preserve_format: same strides as the dense input
        _lib.call("tlxmi_affine_act", _p(x), None, None, None, _p(y), dt_code(x.dtype), n // v, v, v, 0, v, act,
                  float(act_param), 0, _stream())
        return y
    npad = (n + v - 1) // v * v
    buf = torch.zeros(npad, dtype=x.dtype, device=x.device)
    buf[:n] = x.reshape(-1) if x.is_contiguous() else x.permute(0, 2, 3, 1).reshape(-1)
    out = torch.empty_like(buf)
    _lib.call("tlxmi_affine_act", _p(buf), None, None, None, _p(out), dt_code(x.dtype), npad // v, v, v, 0, v, act,
              float(act_param), 0, _stream())
    if x.is_contiguous():
        return out[:n].view(x.shape)
    N, Cc, H, W = x.shape
    return out[:n].view(N, H, W, Cc).permute(0, 3, 1, 2)


def scale_channels(x, s):
    """x (N,H,W,C) * s (N,C) broadcast over pixels (Squeeze-Excitation gate)."""
    need_gpu(x, "input")
    N, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * Cc)
    y = torch.empty_like(x)
    _lib.call("tlxmi_scale_channels", _p(x), _p(s), _p(y), dt_code(x.dtype), N, HW, Cc, Cc, s.shape[-1], Cc, _stream())
    return y


def adaptive_avgpool2d(x, out_hw):
    """(N,H,W,C) -> (N,OH,OW,C), windows as nn.AdaptiveAvgPool2d (vgg.py:36-39)."""
    need_gpu(x, "input")
    N, H, W, Cc = x.shape
    OH, OW = out_hw
    if (OH, OW) == (H, W):
        return x
    y = torch.empty((N, OH, OW, Cc), dtype=x.dtype, device=x.device)
    _lib.call("tlxmi_adaptive_avgpool2d", _p(x), _p(y), dt_code(x.dtype), N, H, W, Cc, OH, OW, x.stride(2), Cc, _stream())
    return y


def layernorm(x, gamma, beta, eps):
    need_gpu(x, "input")
    if not x.is_contiguous():
        x = x.contiguous()
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = torch.empty_like(x)
    _lib.call("tlxmi_layernorm", _p(x), _p(gamma), _p(beta), _p(y), dt_code(x.dtype), rows, Cc, Cc, Cc, float(eps),
              _stream())
    return y


def layernorm_rows(x, rows, Cc, x_ld, gamma, beta, eps):
    """LayerNorm of `rows` rows of width Cc that sit x_ld elements apart in `x` -> dense (rows, Cc)."""
    need_gpu(x, "input")
    y = torch.empty((rows, Cc), dtype=x.dtype, device=x.device)
    _lib.call("tlxmi_layernorm", _p(x), _p(gamma), _p(beta), _p(y), dt_code(x.dtype), rows, Cc, x_ld, Cc,
              float(eps), _stream())
    return y


def broadcast_rows_into(vec_, out, rows, out_ld):
    """out[r*out_ld : r*out_ld + len(vec)] = vec for r < rows (cls-token row of every image)."""
    need_gpu(out, "output")
    Cc = vec_.numel()
    _lib.call("tlxmi_copy_channels", _p(vec_), _p(out), dt_code(out.dtype), rows, Cc, 0, out_ld, _stream())
    return out


def softmax(x, axis=-1):
    """tlx.ops.softmax / nn.Softmax on the device (tlxmi_softmax_rows): fp16 / fp32, any axis (another axis than the last is moved there
    and back: two layout copies)."""
    need_gpu(x, "input")
    if x.dtype not in (torch.float16, torch.float32):
        x = x.to(_precision)
    ax = axis % x.dim()
    if ax != x.dim() - 1:
        return softmax(x.movedim(ax, -1).contiguous(), -1).movedim(-1, ax)
    if not x.is_contiguous():
        x = x.contiguous()
    Cc = x.shape[-1]
    y = torch.empty_like(x)
    if x.numel():
        _lib.call("tlxmi_softmax_rows", _p(x), _p(y), dt_code(x.dtype), x.numel() // Cc, Cc, Cc, Cc, _stream())
    return y


def matmul(a, b, transpose_a=False, transpose_b=False):
    """tlx.matmul on libtlxmi (detr.py:1013 `tlx.matmul(q, k, transpose_b=True)`, vision_transformer.py:117-120): every (M, K) x (K, N)
    product of the broadcast batch is one tlxmi_conv2d launch (a Linear with the second operand packed as its filter) — a coverage path
    for reference-style layer-by-layer forwards (the engine's own models run fused attention kernels); fp16 or fp32, fp32 accumulation."""
    need_gpu(a, "matmul operand")
    need_gpu(b, "matmul operand")
    dt = a.dtype if a.dtype in (torch.float16, torch.float32) else _precision
    a, b = a.to(dt), b.to(dt)
    if a.dim() < 2 or b.dim() < 2:
        raise RuntimeError("matmul: operands of at least two dimensions are expected")
    if transpose_a:
        a = a.transpose(-1, -2)
    w = b if transpose_b else b.transpose(-1, -2)          # (..., N, K): the second operand as a Linear's [out][in] weight
    M, K, N = a.shape[-2], a.shape[-1], w.shape[-2]
    if w.shape[-1] != K:
        raise RuntimeError(f"matmul: inner dimensions {K} and {w.shape[-1]} differ")
    batch = torch.broadcast_shapes(a.shape[:-2], w.shape[:-2])
    a = a.expand(*batch, M, K).reshape(-1, M, K)
    w = w.expand(*batch, N, K).reshape(-1, N, K)
    v = vec(dt)
    Kp = (K + v - 1) // v * v
    if Kp != K:                                            # rows must be whole 16-byte chunks
        a = torch.nn.functional.pad(a, (0, Kp - K))
        w = torch.nn.functional.pad(w, (0, Kp - K))
    a = a.contiguous()
    wf = w.float().contiguous()
    out = torch.empty((a.shape[0], M, N), dtype=dt, device=a.device)
    for i in range(a.shape[0]):
        pk = PackedFilter(wf[i], dt)
        conv2d(a[i].view(M, 1, 1, Kp), pk, out=out[i].view(M, 1, 1, N), out_ld=N)
    return out.view(*batch, M, N)


def attention(qkv, heads, scale, bias=None, mask=None):
    """qkv (B, N, 3*heads*hd) packed as [3][heads][hd] -> (B, N, heads*hd)."""
    need_gpu(qkv, "qkv")
    if not qkv.is_contiguous():
        qkv = qkv.contiguous()
    B, N, C3 = qkv.shape
    hd = C3 // (3 * heads)
    out = torch.empty((B, N, heads * hd), dtype=qkv.dtype, device=qkv.device)
    nW = mask.shape[0] if mask is not None else 0
    d = _lib.AttnDesc(dtype=dt_code(qkv.dtype), B=B, Ntok=N, heads=heads, hd=hd, scale=float(scale), nW=nW)
    _lib.call("tlxmi_attention", C.byref(d), _p(qkv), _p(bias), _p(mask), _p(out), _stream())
    return out


def mha(q, k, v, heads, scale, mask=None, need_weights=False, batch_first=False):
    """General multi-head attention core (tlxmi_mha): q (Lq, B, D), k / v (Lk, B, D) sequence-first — or (B, L, D) with
    batch_first — any row / batch strides as long as the last axis is dense; mask: additive fp32 (Lq, Lk) or
    (B*heads, Lq, Lk).  Returns (out in q's layout, head-averaged weights (B, Lq, Lk) fp32 or None)."""
    for t in (q, k, v):
        need_gpu(t, "mha operand")
        if t.stride(-1) != 1:
            raise RuntimeError("mha: the feature axis must be dense")
    if not (q.dtype == k.dtype == v.dtype):
        raise RuntimeError("mha: q / k / v dtypes differ")
    bd, ld = (0, 1) if batch_first else (1, 0)
    B, Lq, Lk, D = q.shape[bd], q.shape[ld], k.shape[ld], q.shape[-1]
    hd = D // heads
    out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    avg = torch.empty((B, Lq, Lk), dtype=torch.float32, device=q.device) if need_weights else None
    mode = 0
    if mask is not None:
        mask = mask.to(device=q.device, dtype=torch.float32).contiguous()
        if tuple(mask.shape) == (Lq, Lk):
            mode = 1
        elif tuple(mask.shape) == (B * heads, Lq, Lk):
            mode = 2
        else:
            raise RuntimeError(f"mha: attn_mask shape {tuple(mask.shape)}; expected ({Lq}, {Lk}) or ({B * heads}, {Lq}, {Lk})")
    d = _lib.MhaDesc(dtype=dt_code(q.dtype), B=B, Lq=Lq, Lk=Lk, heads=heads, hd=hd, scale=float(scale), mask_mode=mode,
                     q_batch_stride=q.stride(bd), q_row_stride=q.stride(ld), k_batch_stride=k.stride(bd),
                     k_row_stride=k.stride(ld), v_batch_stride=v.stride(bd), v_row_stride=v.stride(ld),
                     out_batch_stride=out.stride(bd), out_row_stride=out.stride(ld))
    _lib.call("tlxmi_mha", C.byref(d), _p(q), _p(k), _p(v), _p(mask), _p(out), _p(avg), _stream())
    return out, avg


def sr_attention(q, kv, heads, scale, fused=None):
    """Spatial-reduction attention (pvt_v2.py:108-146): q (B, Lq, C), kv (B, Lk, 2C) packed [2][heads][hd] as the `kv` Linear leaves it
    -> (B, Lq, C) = softmax(scale * q k^T) v per head, with k = kv[..., :C] and v = kv[..., C:] read in place (two pointers into kv,
    row stride 2C).  tlxmi_sr_attention (MFMA, the scores in registers) when the "sr_attn" option is on, the precision is fp16 and the
    library takes the shape (hd 32 or 64, Lk <= 64); otherwise tlxmi_mha (fp32 always: the parity reference; Lk > 64: a 384 x 384
    input leaves 144 keys).  fused=True / False forces one form (tests, tools/)."""
    need_gpu(q, "q")
    need_gpu(kv, "kv")
    if q.dim() != 3 or kv.dim() != 3 or q.dtype != kv.dtype or kv.shape[0] != q.shape[0] or kv.shape[2] != 2 * q.shape[2] or q.shape[2] % heads:
        raise RuntimeError(f"sr_attention: q (B, Lq, C) and kv (B, Lk, 2C) of one dtype with C a multiple of heads = {heads} are expected, "
                           f"got {tuple(q.shape)} {q.dtype} / {tuple(kv.shape)} {kv.dtype}")
    if q.stride(-1) != 1 or kv.stride(-1) != 1:
        raise RuntimeError("sr_attention: the feature axis must be dense")
    B, Lq, Cc = q.shape
    Lk = kv.shape[1]
    k, v = kv[..., :Cc], kv[..., Cc:]
    out = torch.empty((B, Lq, Cc), dtype=q.dtype, device=q.device)
    es = q.element_size()
    if _sizing():
        _note_act(B * Lq * Cc * es, kv.numel() * es)
    d = _lib.MhaDesc(dtype=dt_code(q.dtype), B=B, Lq=Lq, Lk=Lk, heads=heads, hd=Cc // heads, scale=float(scale), mask_mode=0,
                     q_batch_stride=q.stride(0), q_row_stride=q.stride(1), k_batch_stride=k.stride(0), k_row_stride=k.stride(1),
                     v_batch_stride=v.stride(0), v_row_stride=v.stride(1), out_batch_stride=out.stride(0), out_row_stride=out.stride(1))
    if fused is None:
        fused = bool(_options["sr_attn"] and q.dtype == torch.float16 and _lib.load().tlxmi_sr_attention_supported(C.byref(d))
                     and all(t.data_ptr() % 16 == 0 for t in (q, k, v, out)))

    def launch():
        if fused:
            _lib.call("tlxmi_sr_attention", C.byref(d), _p(q), _p(k), _p(v), _p(out), _stream())
        else:
            _lib.call("tlxmi_mha", C.byref(d), _p(q), _p(k), _p(v), None, _p(out), None, _stream())
    _timed(launch, lambda: ((2 * B * Lq * Cc + 2 * B * Lk * Cc) * es, 4 * B * Lq * Lk * Cc, (B, Lq, Lk, heads, Cc // heads, "sr_attn" if fused else "mha")))
    return out


def gsa_perm(Cc):
    """The contraction order of tlxmi_gsa_block (include/tlxmi.h): a (C / 32, 4, 8) int64 table, perm[s, g, e] = the input channel in slot
    8 g + e of 32-deep step s = 32 s + 4 g + e for e < 4, 32 s + 16 + 4 g + (e - 4) for e >= 4."""
    s = torch.arange(Cc // 32).view(-1, 1, 1)
    g = torch.arange(4).view(1, -1, 1)
    e = torch.arange(8).view(1, 1, -1)
    return 32 * s + 4 * g + (e % 4) + 16 * (e // 4)


def gsa_fragments(w):
    """A Linear weight (in = C, out = C) -> its C * C values in the fragment order of tlxmi_gsa_block: fragment f = ot * (C / 32) + s, lane
    l, element e at f * 512 + l * 8 + e = w[perm(s, l >> 4, e)][16 ot + (l & 15)]."""
    Cc = w.shape[0]
    lane = torch.arange(64)
    rows = gsa_perm(Cc)[:, lane >> 4, :]                                            # (S, 64, 8)
    cols = 16 * torch.arange(Cc // 16).view(-1, 1) + (lane & 15).view(1, -1)        # (CT, 64)
    return w[rows.to(w.device)[None], cols.to(w.device)[:, None, :, None]].reshape(-1)


class GsaBlockParams:
    """The parameters of the attention half of a GSA block (norm1, attn.q, attn.proj), built once per layer by gsa_block_params():
      .block    ONE fp16-element buffer in tlxmi_gsa_block's order (include/tlxmi.h): gamma, beta, bq, bp as fp32 (two elements each), then
                the fragments of Wq and of Wp in fp16; None where the library has no kernel for this width
      .linears  the same layers as engine.layernorm / engine.linear take them (built on first use, per precision): the composition"""

    def __init__(self, gamma, beta, wq, bq, wp, bp):
        Cc = gamma.numel()
        if tuple(wq.shape) != (Cc, Cc) or tuple(wp.shape) != (Cc, Cc) or beta.numel() != Cc or bp.numel() != Cc or (bq is not None and bq.numel() != Cc):
            raise RuntimeError(f"gsa_block_params: norm over {Cc} channels, q {tuple(wq.shape)} and proj {tuple(wp.shape)} (in, out) of that width "
                               "with biases to match are expected")
        f32 = lambda t: t.detach().to(torch.float32).contiguous().view(-1)
        self.C = Cc
        self.gamma, self.beta, self.bp = f32(gamma), f32(beta), f32(bp)
        self.bq = f32(bq) if bq is not None else torch.zeros_like(self.gamma)
        self.wq, self.wp = wq.detach(), wp.detach()
        self.block = None
        if _lib.load().tlxmi_gsa_block_param_count(Cc):
            vecs = torch.cat((self.gamma, self.beta, self.bq, self.bp)).view(torch.float16)
            self.block = torch.cat((vecs, gsa_fragments(self.wq).to(torch.float16), gsa_fragments(self.wp).to(torch.float16))).contiguous()
            if self.block.numel() != _lib.load().tlxmi_gsa_block_param_count(Cc):
                raise RuntimeError("gsa_block_params: the packed size disagrees with the library's")
        self._linears = {}

    def linears(self, dtype):
        hit = self._linears.get(dtype)
        if hit is None:
            hit = (PackedFilter(self.wq.t().contiguous(), dtype), PackedFilter(self.wp.t().contiguous(), dtype))
            self._linears[dtype] = hit
        return hit


def gsa_block_params(norm, q, proj):
    """norm (an nn.LayerNorm: .gamma, .beta), q and proj (nn.Linear: .weights (in, out), .biases or None) -> GsaBlockParams, on the
    device the parameters live on."""
    return GsaBlockParams(norm.gamma, norm.beta, q.weights, q.biases, proj.weights, proj.biases)


def _gsa_desc(x, kv, y, heads, scale, eps):
    Cc = x.shape[2]
    return _lib.GsaBlockDesc(dtype=dt_code(x.dtype), B=x.shape[0], Lq=x.shape[1], Lk=kv.shape[1], C=Cc, heads=heads, scale=float(scale),
                             eps=float(eps), x_batch_stride=x.stride(0), x_row_stride=x.stride(1), k_batch_stride=kv.stride(0),
                             k_row_stride=kv.stride(1), v_batch_stride=kv.stride(0), v_row_stride=kv.stride(1),
                             y_batch_stride=y.stride(0), y_row_stride=y.stride(1))


def _gsa_takes(d, x, kv, y, packed):
    Cc = x.shape[2]
    return bool(_options["gsa_block"] and x.dtype == torch.float16 and kv.dtype == torch.float16 and packed.block is not None
                and packed.block.device == x.device and _lib.load().tlxmi_gsa_block_supported(C.byref(d))
                and all(p_ % 16 == 0 for p_ in (x.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * Cc, y.data_ptr(), packed.block.data_ptr())))


def gsa_block_takes(x, packed, kv, heads, out=None):
    """True where gsa_block(x, packed, kv, heads, ..., out=out) runs as the one fused launch: the "gsa_block" option is on, the tensors are
    fp16 and the library takes the shape.  A model asks before it builds the operands of the composition (the normalised map, q)."""
    y = out if out is not None else x
    return _gsa_takes(_gsa_desc(x, kv, y, int(heads), 1.0, 0.0), x, kv, y, packed)


def gsa_block(x, packed, kv, heads, scale, eps, fused=None, out=None):
    """The attention half of a Twins GSA block (gvt.py:105-127, :148): x (B, Lq, C) the residual stream, kv (B, Lk, 2C) packed
    [2][heads][hd] as the `kv` Linear leaves it (k = kv[..., :C], v = kv[..., C:], read in place), packed = gsa_block_params(norm1, q, proj)
    -> y (B, Lq, C) = x + proj(softmax(scale q k^T) v) with q = q(LayerNorm(x)).  out: the tensor y is written to (x itself updates the
    stream in place).  tlxmi_gsa_block (ONE launch, four MFMA products, x read once and y written once) when the "gsa_block" option is on,
    the tensors are fp16 and the library takes the shape (C 64 / 96 / 128, hd 32 / 64, Lk <= 64); otherwise the composition
    engine.layernorm -> engine.linear -> engine.sr_attention -> engine.linear with the residual (fp32: the parity reference).
    fused=True / False forces one form (tests, tools/); a forced unsupported call raises."""
    need_gpu(x, "x")
    need_gpu(kv, "kv")
    heads = int(heads)
    if (x.dim() != 3 or kv.dim() != 3 or x.dtype != kv.dtype or kv.shape[0] != x.shape[0] or kv.shape[2] != 2 * x.shape[2] or x.shape[2] % heads
            or x.shape[2] != packed.C):
        raise RuntimeError(f"gsa_block: x (B, Lq, C) and kv (B, Lk, 2C) of one dtype with C = {packed.C} a multiple of heads = {heads} are "
                           f"expected, got {tuple(x.shape)} {x.dtype} / {tuple(kv.shape)} {kv.dtype}")
    if x.stride(-1) != 1 or kv.stride(-1) != 1:
        raise RuntimeError("gsa_block: the feature axis must be dense")
    B, Lq, Cc = x.shape
    Lk = kv.shape[1]
    y = out if out is not None else torch.empty((B, Lq, Cc), dtype=x.dtype, device=x.device)
    if tuple(y.shape) != tuple(x.shape) or y.dtype != x.dtype or y.stride(-1) != 1:
        raise RuntimeError("gsa_block: out must have x's shape and dtype and a dense feature axis")
    es = x.element_size()
    if _sizing():
        _note_act(B * Lq * Cc * es, kv.numel() * es)
    k, v = kv[..., :Cc], kv[..., Cc:]
    d = _gsa_desc(x, kv, y, heads, scale, eps)
    if fused is None:
        fused = _gsa_takes(d, x, kv, y, packed)
    if fused:
        if packed.block is None or packed.block.device != x.device:
            raise RuntimeError(f"gsa_block: no packed parameter block for C = {Cc} on {x.device}")
        _timed(lambda: _lib.call("tlxmi_gsa_block", C.byref(d), _p(x), _p(k), _p(v), _p(packed.block), _p(y), _stream()),
               lambda: ((2 * B * Lq * Cc + 2 * B * Lk * Cc) * es + packed.block.numel() * 2, 4 * B * Lq * Cc * Cc + 4 * B * Lq * Lk * Cc,
                        (B, Lq, Lk, heads, Cc // heads, "gsa_block")))
        return y
    pkq, pkp = packed.linears(x.dtype)
    xc = x if x.is_contiguous() else x.contiguous()
    q = linear(layernorm(xc, packed.gamma, packed.beta, eps), pkq, packed.bq)
    o = sr_attention(q, kv, heads, scale)
    if out is None:
        return linear(o, pkp, packed.bp, res=xc)
    if out.is_contiguous():
        linear(o, pkp, packed.bp, res=xc, out=out)
    else:
        out.copy_(linear(o, pkp, packed.bp, res=xc))
    return out


def cswin_stripes(H, W, splits):
    """The stripe (height, width) of each branch: `splits` = one (hs, ws) pair per branch, or an int s for CSWin's pair of a vertical
    (H, s) and a horizontal (s, W) stripe (cswin_transformer.py:263-273)."""
    if isinstance(splits, int):
        return [(H, splits), (splits, W)]
    return [(int(a), int(b)) for a, b in splits]


def _cswin_desc(dtype, B, H, W, heads, hd, stripes, scale, q, k, v, out):
    hs = (C.c_int32 * 2)(*([s[0] for s in stripes] + [0])[:2])
    ws = (C.c_int32 * 2)(*([s[1] for s in stripes] + [0])[:2])
    return _lib.CswinAttnDesc(dtype=dt_code(dtype), B=B, H=H, W=W, hd=hd, scale=float(scale), branches=len(stripes), heads=heads // len(stripes),
                              hs=hs, ws=ws, q_batch_stride=q.stride(0), q_row_stride=q.stride(1), k_batch_stride=k.stride(0),
                              k_row_stride=k.stride(1), v_batch_stride=v.stride(0), v_row_stride=v.stride(1),
                              out_batch_stride=out.stride(0), out_row_stride=out.stride(1))


def cswin_attention(qkv, B, H, W, heads, splits, w_lepe, b_lepe, scale, fused=None):
    """CSWin's attention of one block (cswin_transformer.py:151-222, :285-300): qkv (B, H*W, 3C) packed [3][heads][hd] as the `qkv`
    Linear leaves it, token (y, x) = row y*W + x -> (B, H*W, C).  `heads` heads in all, split evenly over the branches of `splits`
    (cswin_stripes: an int s = the (H, s) and (s, W) stripes; a list of (hs, ws) pairs, one per branch); each head attends inside the
    stripes of its branch and adds LePE, the depthwise 3x3 of V inside the stripe: w_lepe [3][3][C] in qkv's dtype (both branches'
    channels side by side), b_lepe fp32 [C] or None.  q, k, v are three pointers into qkv (row stride 3C), read in place.
    tlxmi_cswin_attention (MFMA, the scores in registers) when the "cswin_attn" option is on, the precision is fp16, the library takes
    the shape (hd 32, stripes of at most 128 tokens) and the pointers are 16-byte aligned; otherwise tlxmi_cswin_attention_plain (fp32
    always: the parity reference).  fused=True / False forces one form (tests, tools/); a forced unsupported call raises."""
    need_gpu(qkv, "qkv")
    stripes = cswin_stripes(H, W, splits)
    nb = len(stripes)
    if qkv.dim() != 3 or qkv.shape[0] != B or qkv.shape[1] != H * W or qkv.shape[2] % (3 * heads) or nb not in (1, 2) or heads % nb:
        raise RuntimeError(f"cswin_attention: qkv (B, H*W, 3C) = ({B}, {H * W}, 3C) with C a multiple of heads = {heads} and 1 or 2 branches "
                           f"that split the heads evenly are expected, got {tuple(qkv.shape)} and {nb} branches")
    if qkv.stride(-1) != 1:
        raise RuntimeError("cswin_attention: the feature axis must be dense")
    Cc = qkv.shape[2] // 3
    if tuple(w_lepe.shape) != (3, 3, Cc) or w_lepe.dtype != qkv.dtype or not w_lepe.is_contiguous():
        raise RuntimeError(f"cswin_attention: a dense [3][3][{Cc}] LePE filter of qkv's dtype is expected, got {tuple(w_lepe.shape)} {w_lepe.dtype}")
    if b_lepe is not None and (tuple(b_lepe.shape) != (Cc,) or b_lepe.dtype != torch.float32 or not b_lepe.is_contiguous()):
        raise RuntimeError(f"cswin_attention: the LePE bias is fp32 [{Cc}]")
    for hs, ws in stripes:
        if hs < 1 or ws < 1 or H % hs or W % ws:
            raise RuntimeError(f"cswin_attention: a {hs} x {ws} stripe does not divide the {H} x {W} image")
    q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
    out = torch.empty((B, H * W, Cc), dtype=qkv.dtype, device=qkv.device)
    es = qkv.element_size()
    if _sizing():
        _note_act(out.numel() * es, qkv.numel() * es)
    hd = Cc // heads
    d = _cswin_desc(qkv.dtype, B, H, W, heads, hd, stripes, scale, q, k, v, out)
    if fused is None:
        fused = bool(_options["cswin_attn"] and qkv.dtype == torch.float16 and _lib.load().tlxmi_cswin_attention_supported(C.byref(d))
                     and all(t.data_ptr() % 16 == 0 for t in (q, k, v, out, w_lepe) + ((b_lepe,) if b_lepe is not None else ())))

    def entry():
        keys = sum(hs * ws for hs, ws in stripes) / nb                  # keys a query meets, averaged over the branches
        return (4 * B * H * W * Cc * es + w_lepe.numel() * es, int(4 * B * H * W * keys * Cc) + 18 * B * H * W * Cc,
                (B, H, W, heads, hd, tuple(stripes), "cswin_attn" if fused else "cswin_plain"))
    _timed(lambda: _lib.call("tlxmi_cswin_attention" if fused else "tlxmi_cswin_attention_plain", C.byref(d), _p(q), _p(k), _p(v), _p(w_lepe),
                             _p(b_lepe), _p(out), _stream()), entry)
    return out


def levit_bias_grid(attention_biases, Rq, Rk, stride):
    """LeViT's `attention_biases` parameter (heads, n_offsets) -> the fp32 [heads][Rk][Rk] grid tlxmi_levit_attention indexes by
    (|dy|, |dx|) on the key grid.  Column n of the parameter is the n-th DISTINCT offset in the order the reference's dictionary loop
    meets them (levit.py:172-181 for a stage, :270-283 for a subsample layer: queries row-major outside, keys row-major inside, offset
    (|y_q*stride - y_k|, |x_q*stride - x_k|)); offsets that never occur stay zero."""
    if attention_biases.dim() != 2:
        raise RuntimeError(f"levit_bias_grid: a (heads, n_offsets) parameter is expected, got {tuple(attention_biases.shape)}")
    Rq, Rk, stride = int(Rq), int(Rk), int(stride)
    if Rq < 1 or Rk < 1 or stride < 1 or (Rq - 1) * stride > Rk - 1:
        raise RuntimeError(f"levit_bias_grid: a {Rq} x {Rq} query grid at stride {stride} does not sit on a {Rk} x {Rk} key grid")
    order = {}
    for qy in range(Rq):
        for qx in range(Rq):
            for ky in range(Rk):
                for kx in range(Rk):
                    off = (abs(qy * stride - ky), abs(qx * stride - kx))
                    if off not in order:
                        order[off] = len(order)
    if attention_biases.shape[1] != len(order):
        raise RuntimeError(f"levit_bias_grid: {attention_biases.shape[1]} offsets in the parameter, the grids have {len(order)}")
    dy = torch.tensor([o[0] for o in order], dtype=torch.long, device=attention_biases.device)
    dx = torch.tensor([o[1] for o in order], dtype=torch.long, device=attention_biases.device)
    grid = torch.zeros((attention_biases.shape[0], Rk, Rk), dtype=torch.float32, device=attention_biases.device)
    grid[:, dy, dx] = attention_biases.detach().float()
    return grid.contiguous()


def _levit_desc(dtype, B, heads, kd, d, Rq, Rk, stride, scale, act, q, k, v, out, q_hs, k_hs, v_hs):
    return _lib.LevitAttnDesc(dtype=dt_code(dtype), B=B, heads=heads, kd=kd, d=d, Rq=Rq, Rk=Rk, stride=stride, scale=float(scale), act=int(act),
                              q_batch_stride=q.stride(0), q_row_stride=q.stride(1), q_head_stride=q_hs,
                              k_batch_stride=k.stride(0), k_row_stride=k.stride(1), k_head_stride=k_hs,
                              v_batch_stride=v.stride(0), v_row_stride=v.stride(1), v_head_stride=v_hs,
                              out_batch_stride=out.stride(0), out_row_stride=out.stride(1))


def levit_attention(kv, bias_grid, heads, kd, d, Rk, scale, q=None, Rq=None, stride=1, act=ACT_HARDSWISH, fused=None):
    """LeViT's attention (levit.py:199-224, :301-323) -> (B, Rq*Rq, heads*d), `act` (ACT_NONE or ACT_HARDSWISH, the activation in front
    of `proj`) applied.  Token (y, x) of an R x R grid is row y*R + x.
      a stage (q=None):   kv is the packed `qkv` rows (B, Rk*Rk, heads*(2kd + d)), [heads][kd | kd | d] per row; Rq = Rk, stride 1;
      a subsample layer:  q (B, Rq*Rq, heads*kd) and kv the packed `kv` rows (B, Rk*Rk, heads*(kd + d)), [heads][kd | d] per row; query
                          (y, x) sits at key-grid position (y*stride, x*stride).
    q, k, v are pointers into those rows, read in place.  bias_grid: fp32 [heads][Rk][Rk] (levit_bias_grid).
    tlxmi_levit_attention (MFMA, the scores in registers) when the "levit_attn" option is on, the precision is fp16, the library takes the
    shape (kd 16 / 32, d 32 / 64 / 128, Rk <= 16) and the pointers are 16-byte aligned; otherwise tlxmi_levit_attention_plain (fp32
    arithmetic: the parity reference).  fused=True / False forces one form (tests, tools/); a forced unsupported call raises."""
    need_gpu(kv, "kv")
    heads, kd, d, Rk, stride = int(heads), int(kd), int(d), int(Rk), int(stride)
    per = (kd + d) if q is not None else (2 * kd + d)
    if kv.dim() != 3 or kv.shape[1] != Rk * Rk or kv.shape[2] != heads * per or kv.stride(-1) != 1:
        raise RuntimeError(f"levit_attention: packed rows (B, {Rk * Rk}, {heads * per}) with a dense feature axis are expected, got "
                           f"{tuple(kv.shape)}")
    B = kv.shape[0]
    if q is None:
        Rq, stride = Rk, 1
        qv, kview, vview, q_hs = kv, kv[..., kd:], kv[..., 2 * kd:], per
    else:
        need_gpu(q, "q")
        Rq = int(Rq)
        if q.dim() != 3 or tuple(q.shape) != (B, Rq * Rq, heads * kd) or q.stride(-1) != 1 or q.dtype != kv.dtype:
            raise RuntimeError(f"levit_attention: q ({B}, {Rq * Rq}, {heads * kd}) of kv's dtype with a dense feature axis is expected, got "
                               f"{tuple(q.shape)} {q.dtype}")
        qv, kview, vview, q_hs = q, kv, kv[..., kd:], kd
    if (Rq - 1) * stride > Rk - 1 or Rq < 1 or stride < 1:
        raise RuntimeError(f"levit_attention: a {Rq} x {Rq} query grid at stride {stride} does not sit on a {Rk} x {Rk} key grid")
    if tuple(bias_grid.shape) != (heads, Rk, Rk) or bias_grid.dtype != torch.float32 or not bias_grid.is_contiguous() or not bias_grid.is_cuda:
        raise RuntimeError(f"levit_attention: a dense fp32 [{heads}][{Rk}][{Rk}] bias grid on the device is expected, got "
                           f"{tuple(bias_grid.shape)} {bias_grid.dtype}")
    if act not in (ACT_NONE, ACT_HARDSWISH):
        raise RuntimeError("levit_attention: act is ACT_NONE or ACT_HARDSWISH")
    out = torch.empty((B, Rq * Rq, heads * d), dtype=kv.dtype, device=kv.device)
    es = kv.element_size()
    if _sizing():
        _note_act(out.numel() * es, kv.numel() * es)
    dsc = _levit_desc(kv.dtype, B, heads, kd, d, Rq, Rk, stride, scale, act, qv, kview, vview, out, q_hs, per, per)
    if fused is None:
        fused = bool(_options["levit_attn"] and kv.dtype == torch.float16 and _lib.load().tlxmi_levit_attention_supported(C.byref(dsc))
                     and all(t.data_ptr() % 16 == 0 for t in (qv, kview, vview, out, bias_grid)))
    Lq, Lk = Rq * Rq, Rk * Rk
    _timed(lambda: _lib.call("tlxmi_levit_attention" if fused else "tlxmi_levit_attention_plain", C.byref(dsc), _p(qv), _p(kview), _p(vview),
                             _p(bias_grid), _p(out), _stream()),
           lambda: (B * heads * (Lq * kd + Lk * (kd + d) + Lq * d) * es + heads * Lk * 4, 2 * B * heads * Lq * Lk * (kd + d),
                    (B, Rq, Rk, stride, heads, kd, d, "levit_attn" if fused else "levit_plain")))
    return out


TNT_INNER_NAMES = ("norm_in.gamma", "norm_in.beta", "attn_in.qk.weights", "attn_in.v.weights", "attn_in.proj.weights", "attn_in.proj.biases",
                   "norm_mlp_in.gamma", "norm_mlp_in.beta", "mlp_in.fc1.weights", "mlp_in.fc1.biases", "mlp_in.fc2.weights", "mlp_in.fc2.biases",
                   "norm1_proj.gamma", "norm1_proj.beta")


def tnt_inner_params(block_params):
    """The inner half of a TNT block's parameters (a mapping from the names in TNT_INNER_NAMES, relative to the block, to tensors; weights
    (in, out) as nn.Linear keeps them) -> ONE fp32 device buffer in the order tlxmi_tnt_inner reads (include/tlxmi.h):
    g1 b1 | Wqk | Wv | Wproj bproj | g2 b2 | Wfc1 bfc1 | Wfc2 bfc2 | g3 b3.  `qk` and `v` carry no bias (tnt.py:83-87)."""
    missing = [n for n in TNT_INNER_NAMES if n not in block_params]
    if missing:
        raise RuntimeError(f"tnt_inner_params: missing {missing}")
    t = {n: block_params[n].detach() for n in TNT_INNER_NAMES}
    D = t["norm_in.gamma"].numel()
    hid = t["mlp_in.fc1.biases"].numel()
    want = {"attn_in.qk.weights": (D, 2 * D), "attn_in.v.weights": (D, D), "attn_in.proj.weights": (D, D), "attn_in.proj.biases": (D,),
            "mlp_in.fc1.weights": (D, hid), "mlp_in.fc2.weights": (hid, D), "mlp_in.fc2.biases": (D,)}
    want.update({n: (D,) for n in TNT_INNER_NAMES if n.endswith((".gamma", ".beta"))})
    for n, shp in want.items():
        if tuple(t[n].shape) != shp:
            raise RuntimeError(f"tnt_inner_params: {n} is {tuple(t[n].shape)}, expected {shp}")
    buf = torch.cat([t[n].float().reshape(-1) for n in TNT_INNER_NAMES]).contiguous()
    if buf.numel() != _lib.load().tlxmi_tnt_inner_param_count(D, hid):
        raise RuntimeError("tnt_inner_params: the packed size disagrees with the library's")
    return buf


def _tnt_desc(dtype, patches, pixels, dim, heads, hidden, eps, x_ld, y_ld, yn_ld):
    return _lib.TntInnerDesc(dtype=dt_code(dtype), patches=patches, pixels=pixels, dim=dim, heads=heads, hidden=hidden,
                             scale=float((dim // heads) ** -0.5), eps1=float(eps[0]), eps2=float(eps[1]), eps3=float(eps[2]),
                             x_row_stride=x_ld, y_row_stride=y_ld, yn_row_stride=yn_ld)


def tnt_inner(x, packed, heads, eps_in=1e-5, eps_mlp=1e-5, eps_proj=1e-5, y_norm=True, fused=None, out=None):
    """The inner half of a TNT block (tnt.py:142-149) on x (patches, pixels, dim) -> (y, y_norm): y = x + proj(attn(LN(x))), then
    y + fc2(gelu(fc1(LN(y)))); y_norm (patches, pixels*dim) = the third LayerNorm of y, flattened pixel-major (None when y_norm is False).
    packed: tnt_inner_params(...).  out: the tensor y is written to (x itself updates the map in place).
    tlxmi_tnt_inner (one launch, every product on MFMA) when the "tnt_inner" option is on, the precision is fp16 and the library takes the
    shape (16 pixels, dim 24, 4 heads, hidden 96); otherwise tlxmi_tnt_inner_plain (fp32 arithmetic: the parity reference).
    fused=True / False forces one form (tests, tools/); a forced unsupported call raises."""
    need_gpu(x, "x")
    heads = int(heads)
    if x.dim() != 3 or x.stride(-1) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        raise RuntimeError(f"tnt_inner: (patches, pixels, dim) rows with a dense channel axis and evenly spaced rows are expected, got "
                           f"{tuple(x.shape)} strides {tuple(x.stride())}")
    patches, pixels, D = x.shape
    if heads < 1 or D % heads:
        raise RuntimeError(f"tnt_inner: {heads} heads do not divide dim {D}")
    rest = packed.numel() - 4 * D * D - 8 * D
    if packed.dtype != torch.float32 or not packed.is_cuda or not packed.is_contiguous() or rest <= 0 or rest % (2 * D + 1):
        raise RuntimeError(f"tnt_inner: a dense fp32 device buffer from tnt_inner_params for dim {D} is expected, got {tuple(packed.shape)} {packed.dtype}")
    hidden = rest // (2 * D + 1)
    y = out if out is not None else torch.empty((patches, pixels, D), dtype=x.dtype, device=x.device)
    if (tuple(y.shape) != tuple(x.shape) or y.dtype != x.dtype or y.stride(-1) != 1 or y.stride(0) != pixels * y.stride(1)):
        raise RuntimeError("tnt_inner: out must have x's shape and dtype, a dense channel axis and evenly spaced rows")
    yn = torch.empty((patches, pixels * D), dtype=x.dtype, device=x.device) if y_norm else None
    es = x.element_size()
    if _sizing():
        _note_act(x.numel() * es)
    dsc = _tnt_desc(x.dtype, patches, pixels, D, heads, hidden, (eps_in, eps_mlp, eps_proj), x.stride(1), y.stride(1), pixels * D)
    if fused is None:
        fused = bool(_options["tnt_inner"] and x.dtype == torch.float16 and _lib.load().tlxmi_tnt_inner_supported(C.byref(dsc))
                     and all(t_.data_ptr() % 16 == 0 for t_ in (x, y, packed) + ((yn,) if yn is not None else ())))
    _timed(lambda: _lib.call("tlxmi_tnt_inner" if fused else "tlxmi_tnt_inner_plain", C.byref(dsc), _p(x), _p(packed), _p(y), _p(yn), _stream()),
           lambda: (patches * pixels * D * es * (3 if y_norm else 2) + packed.numel() * 4,
                    2 * patches * pixels * (4 * D * D + 2 * D * hidden + 2 * heads * pixels * (D // heads)),
                    (patches, pixels, D, heads, "tnt_inner" if fused else "tnt_plain")))
    return y, yn


def yolo_box(heads_nhwc, anchors, num_classes, img_size, conf_thresh=0.005, downsample_ratio=32, clip_bbox=True, scale_x_y=1.0):
    """YOLOBox.__call__ (yolov3.py:558-579) on the device: `heads_nhwc` are the head maps (N,H,W,A*(5+C)) from the coarsest
    stride down, `anchors` the flat (w, h, w, h, ...) list per head (YOLOv3Head.mask_anchors), img_size (N,2) int32 (h, w).
    -> boxes (N, M, 4) fp32, scores (N, M, C) fp32 with M = sum A*H*W, heads appended in order."""
    N = heads_nhwc[0].shape[0]
    As = [len(a) // 2 for a in anchors]
    Ms = [A * h.shape[1] * h.shape[2] for A, h in zip(As, heads_nhwc)]
    Mtot = sum(Ms)
    dev = heads_nhwc[0].device
    boxes = torch.empty((N, Mtot, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((N, Mtot, num_classes), dtype=torch.float32, device=dev)
    img = img_size.to(device=dev, dtype=torch.int32).contiguous()
    off = 0
    for i, (h, anc) in enumerate(zip(heads_nhwc, anchors)):
        need_gpu(h, "head map")
        if not h.is_contiguous() or h.shape[-1] != As[i] * (5 + num_classes):
            raise RuntimeError(f"yolo_box: head {i} must be a dense (N,H,W,{As[i] * (5 + num_classes)}) map")
        a = torch.tensor(anc, dtype=torch.float32, device=dev)
        _lib.call("tlxmi_yolo_box", _p(h), dt_code(h.dtype), N, As[i], num_classes, h.shape[1], h.shape[2], 1, _p(img), _p(a),
                  C.c_float(conf_thresh), int(downsample_ratio // 2 ** i), 1 if clip_bbox else 0, C.c_float(scale_x_y), _p(boxes), _p(scores),
                  Mtot, off, _stream())
        off += Ms[i]
    return boxes, scores


def yolo_iou_aware(head_nhwc, num_anchors, num_classes, factor):
    """YOLOv3Head's IoU-aware objectness (yolov3.py:355-376) on one NHWC head map (N,H,W,A*(6+C)) -> (N,H,W,A*(5+C))."""
    need_gpu(head_nhwc, "head map")
    N, H, W, Cc = head_nhwc.shape
    if Cc != num_anchors * (6 + num_classes) or not head_nhwc.is_contiguous():
        raise RuntimeError(f"yolo_iou_aware: a dense (N,H,W,{num_anchors * (6 + num_classes)}) map is expected")
    y = torch.empty((N, H, W, num_anchors * (5 + num_classes)), dtype=head_nhwc.dtype, device=head_nhwc.device)
    _lib.call("tlxmi_yolo_iou_aware", _p(head_nhwc), _p(y), dt_code(head_nhwc.dtype), N * H * W, int(num_anchors), int(num_classes),
              C.c_float(factor), _stream())
    return y


def multiclass_nms(boxes, scores, score_threshold=0.05, nms_threshold=0.5, keep_top_k=100, return_index=False):
    """tlx_multiclass_nms (detection/utils/ops.py:255-329) on the device: boxes (N,M,4), scores (N,M,C) fp32 ->
    (detections (N, keep_top_k, 6) rows (class, score, x1, y1, x2, y2), counts (N,) int32); return_index (yolov3.py:70-78, the
    for_mot post-process): also keep_index (N, keep_top_k) int32, each row's box among the M of its image, -1 past the count."""
    need_gpu(boxes, "boxes")
    boxes, scores = boxes.float().contiguous(), scores.float().contiguous()
    N, M, Cc = scores.shape
    ws = torch.empty(_lib.load().tlxmi_multiclass_nms_workspace_bytes(N, M), dtype=torch.uint8, device=boxes.device)
    det = torch.empty((N, keep_top_k, 6), dtype=torch.float32, device=boxes.device)
    cnt = torch.empty((N,), dtype=torch.int32, device=boxes.device)
    if return_index:
        idx = torch.empty((N, keep_top_k), dtype=torch.int32, device=boxes.device)
        _lib.call("tlxmi_multiclass_nms_index", _p(boxes), _p(scores), N, M, Cc, C.c_float(score_threshold), C.c_float(nms_threshold),
                  int(keep_top_k), _p(ws), _p(det), _p(cnt), _p(idx), _stream())
        return det, cnt, idx
    _lib.call("tlxmi_multiclass_nms", _p(boxes), _p(scores), N, M, Cc, C.c_float(score_threshold), C.c_float(nms_threshold), int(keep_top_k),
              _p(ws), _p(det), _p(cnt), _stream())
    return det, cnt


def attention_table(bias, mask, N):
    """bias (heads, N, N) + mask (nW, N, N) or None -> the pre-summed, padded table of tlxmi_attention_comb:
    (max(nW,1), heads, NP, NP) fp32, NP = 32 * ceil(N / 32).  Built once per layer (the reference adds the two on
    every forward, swin_transformer.py:205-220)."""
    NP = (N + 31) // 32 * 32
    nW = mask.shape[0] if mask is not None else 1
    t = torch.zeros((nW, bias.shape[0], NP, NP), dtype=torch.float32, device=bias.device)
    t[:, :, :N, :N] = bias.float()[None]
    if mask is not None:
        t[:, :, :N, :N] += mask.float().to(bias.device)[:, None]
    return t.contiguous()


def attention_comb(qkv, heads, scale, table, nW):
    """attention() with a table from attention_table(); fp16, head dim 32 / 64 / 96, N <= 256."""
    need_gpu(qkv, "input")
    B, N, C3 = qkv.shape
    hd = C3 // (3 * heads)
    out = torch.empty((B, N, heads * hd), dtype=qkv.dtype, device=qkv.device)
    d = _lib.AttnDesc(dtype=dt_code(qkv.dtype), B=B, Ntok=N, heads=heads, hd=hd, scale=float(scale), nW=nW)
    _lib.call("tlxmi_attention_comb", C.byref(d), _p(qkv), _p(table), _p(out), _stream())
    return out


def attention_windows(qkv, heads, scale, table, nW, H, W, ws, shift):
    """Swin's windowed attention on IMAGE-order rows (tlxmi_attention_windows): qkv (B, H * W, 3 * heads * hd) -> (B, H * W, heads * hd); the
    cyclic shift and the window partition / reverse (swin_transformer.py:316-333) are row arithmetic inside the kernel.  table:
    attention_table(); nW: 0 or the windows per image (with the shift mask in the table)."""
    need_gpu(qkv, "qkv")
    B, L, C3 = qkv.shape
    hd = C3 // (3 * heads)
    out = torch.empty((B, L, heads * hd), dtype=qkv.dtype, device=qkv.device)
    wpi = (H // ws) * (W // ws)
    d = _lib.AttnDesc(dtype=dt_code(qkv.dtype), B=B * wpi, Ntok=ws * ws, heads=heads, hd=hd, scale=float(scale), nW=nW)
    _lib.call("tlxmi_attention_windows", C.byref(d), _p(qkv), _p(table), _p(out), H, W, ws, shift, _stream())
    return out


def window_partition(x, ws, shift):
    """(B,H,W,C) -> (B*nW, ws*ws, C) with the cyclic shift folded in."""
    need_gpu(x, "input")
    B, H, W, Cc = x.shape
    y = torch.empty((B * (H // ws) * (W // ws), ws * ws, Cc), dtype=x.dtype, device=x.device)
    _lib.call("tlxmi_window_partition", _p(x), _p(y), dt_code(x.dtype), B, H, W, Cc, ws, shift, _stream())
    return y


def window_reverse(win, B, H, W, ws, shift, res=None):
    need_gpu(win, "input")
    Cc = win.shape[-1]
    y = torch.empty((B, H, W, Cc), dtype=win.dtype, device=win.device)
    _lib.call("tlxmi_window_reverse", _p(win), _p(res), _p(y), dt_code(win.dtype), B, H, W, Cc, ws, shift, _stream())
    return y


def layernorm_window_partition(x, gamma, beta, eps, ws, shift):
    """(B,H,W,C) -> window_partition(roll(LayerNorm(x), -shift)) as (B*nW, ws*ws, C) in one pass."""
    need_gpu(x, "input")
    B, H, W, Cc = x.shape
    y = torch.empty((B * (H // ws) * (W // ws), ws * ws, Cc), dtype=x.dtype, device=x.device)
    _lib.call("tlxmi_layernorm_window_partition", _p(x), _p(_f32(gamma)), _p(_f32(beta)), _p(y), dt_code(x.dtype), B, H, W, Cc,
              ws, shift, C.c_float(eps), _stream())
    return y


def window_reverse_layernorm(win, res, gamma, beta, eps, ws, shift):
    """sum = res + roll(window_reverse(win), +shift); returns (sum, LayerNorm(sum)), both (B,H,W,C), in one pass."""
    need_gpu(win, "input")
    B, H, W, Cc = res.shape
    s = torch.empty_like(res)
    y = torch.empty_like(res)
    _lib.call("tlxmi_window_reverse_layernorm", _p(win), _p(res), _p(_f32(gamma)), _p(_f32(beta)), _p(s), _p(y),
              dt_code(win.dtype), B, H, W, Cc, ws, shift, C.c_float(eps), _stream())
    return s, y


def patch_merge_layernorm(x, gamma, beta, eps):
    """(B,H,W,C) -> LayerNorm over 4C of PatchMerging's 2 x 2 gather + concat, (B, H/2 * W/2, 4C), in one pass."""
    need_gpu(x, "input")
    B, H, W, Cc = x.shape
    y = torch.empty((B, (H // 2) * (W // 2), 4 * Cc), dtype=x.dtype, device=x.device)
    _lib.call("tlxmi_patch_merge_layernorm", _p(x), _p(_f32(gamma)), _p(_f32(beta)), _p(y), dt_code(x.dtype), B, H, W, Cc,
              C.c_float(eps), _stream())
    return y


def patch_merge_gather(x):
    need_gpu(x, "input")
    B, H, W, Cc = x.shape
    y = torch.empty((B, H // 2, W // 2, 4 * Cc), dtype=x.dtype, device=x.device)
    _lib.call("tlxmi_patch_merge_gather", _p(x), _p(y), dt_code(x.dtype), B, H, W, Cc, _stream())
    return y


def upsample2x_into(x, out, c_off):
    need_gpu(x, "input")
    N, H, W, Cc = x.shape
    _lib.call("tlxmi_upsample2x_nearest", _p(x), _p(out), dt_code(x.dtype), N, H, W, Cc, Cc, out.shape[-1], c_off,
              _stream())
    return out


def copy_channels_into(x, out, c_off, x_ld=None):
    """out[..., c_off:c_off+C] = x   (tlx.concat along channels, one pass per source).
    x_ld: the pixel pitch when x is a column slice of a wider map (a view: its last axis is the slice's width)."""
    need_gpu(x, "input")
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    es = x.element_size()
    dst = C.c_void_p(out.data_ptr() + c_off * es)
    _lib.call("tlxmi_copy_channels", _p(x), dst, dt_code(x.dtype), rows, Cc, Cc if x_ld is None else int(x_ld), out.shape[-1], _stream())
    return out


def argmax_lastdim(x):
    need_gpu(x, "input")
    if not x.is_contiguous():
        x = x.contiguous()
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    out = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
    _lib.call("tlxmi_argmax_lastdim", _p(x), dt_code(x.dtype), rows, Cc, Cc, _p(out), _stream())
    return out


def resize_out_size(n_in, scale):
    """Output extent of torch.nn.functional.interpolate(scale_factor=scale) along one axis: floor(n_in * scale) in double."""
    import math
    return int(math.floor(float(n_in) * float(scale)))


def resize_bilinear(x, scale, align_corners=False, channels=None, out=None, layout="nhwc", out_dtype=None):
    """Bilinear resize (tlx.Resize(method="bilinear"), deeplab.py:177-182) of an NHWC map x (N, H, W, x_ld), `channels` of its
    x_ld used (default all).  scale: s or (sh, sw) as interpolate(scale_factor=) takes it -> (floor(H * sh), floor(W * sw)).
    layout "nhwc": y (N, Ho, Wo, C), or written into `out` — an (N, Ho, Wo, C) view with unit channel stride, e.g. a column
    slice of a wider buffer (the ASPP concat); "nchw": a dense (N, C, Ho, Wo) tensor.  fp32 interpolation; out_dtype fp16 / fp32
    (default x's)."""
    need_gpu(x, "input")
    N, H, W, ld = x.shape
    if not x.is_contiguous():
        raise RuntimeError("resize_bilinear: x must be a dense NHWC map (N, H, W, x_ld)")
    Cc = ld if channels is None else int(channels)
    sh, sw = (scale, scale) if isinstance(scale, (int, float)) else (scale[0], scale[1])
    Ho, Wo = resize_out_size(H, sh), resize_out_size(W, sw)
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError(f"resize_bilinear: empty output {Ho}x{Wo} for input {H}x{W} at scale {scale}")
    dt = out_dtype or (out.dtype if out is not None else x.dtype)
    nstride = 0
    if layout == "nchw":
        if out is not None:
            raise RuntimeError("resize_bilinear: the NCHW form allocates its output")
        out = torch.empty((N, Cc, Ho, Wo), dtype=dt, device=x.device)
        y_ld, lay = 0, _lib.LAYOUT_NCHW
    elif layout == "nhwc":
        if out is None:
            out = torch.empty((N, Ho, Wo, Cc), dtype=dt, device=x.device)
        # pixel pitch / image stride of the view (strides of size-1 axes carry no meaning)
        y_ld = out.stride(2) if Wo > 1 else out.stride(1) if Ho > 1 else Cc
        nstride = out.stride(0) if N > 1 else Ho * Wo * y_ld
        if (tuple(out.shape) != (N, Ho, Wo, Cc) or out.dtype != dt or (Cc > 1 and out.stride(3) != 1) or y_ld < Cc
                or (Ho > 1 and Wo > 1 and out.stride(1) != Wo * y_ld)):
            raise RuntimeError(f"resize_bilinear: out must be an ({N}, {Ho}, {Wo}, {Cc}) {dt} view with rows of one pitch")
        lay = _lib.LAYOUT_NHWC
    else:
        raise ValueError(f"resize_bilinear: layout {layout!r}")
    _lib.call("tlxmi_resize_bilinear", _p(x), dt_code(x.dtype), N, H, W, Cc, ld, _p(out), dt_code(dt), Ho, Wo, lay, y_ld, nstride,
              1 if align_corners else 0, float(sh), float(sw), _stream())
    return out
