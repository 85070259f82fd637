"""Generate tests/golden/*.npz — run ONLY in the development container (needs /root/reference).

Every fixture is one entry of `jobs()`.  For a model fixture (`Job`) `write` does, in this order:
  1. import the reference model file UNMODIFIED from /root/reference by path (`reference`), with `tensorlayerx` resolved to the
     oracle's torch-CPU stand-in (oracle/tlx_cpu) and, for the Paddle-converted files and detection/yolov3.py, the packages they
     hard-import and this image lacks (paddle, paddle2tlx, decorator, torchvision) resolved to the import shims of oracle/shims/
     (README there lists what each provides) — the reference source is never copied;
  2. fill the model and the restatement (oracle/functional.py, tests/*_restated.py) from the same seeded numpy recipe;
  3. require restatement == reference graph (max abs diff <= 1e-5, same argmax);
  4. try the job's seeds in order until its acceptance rules hold: top-1 margins above 2 x the bound on every row (or on half of
     the rows), every recorded intermediate below 1000 in magnitude (fp16 headroom), rows that do not share one argmax;
  5. write the fixture: recipe ids + expected outputs.
The stand-in and the shims provide whatever the reference files use; nothing is patched in here, so a fixture does not depend on
what was generated before it in the process.

    python -m oracle.gen_golden                     # writes every fixture of tests/golden/
    python -m oracle.gen_golden swin yolo           # only the fixtures whose file name contains one of the words, in that order
    python -m oracle.gen_golden --check [words]     # writes to a temporary directory and compares with the committed fixtures
"""
import dataclasses
import importlib
import importlib.util
import os
import sys
import tempfile
import time
import types
from functools import partial
from typing import Callable

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REF = "/root/reference"
GOLDEN = os.path.join(REPO, "tests", "golden")
TESTS = os.path.join(REPO, "tests")

from oracle import functional as OF  # noqa: E402
from oracle.tlx_cpu import pd  # noqa: E402
from tlxcv_amd import seeded  # noqa: E402


SHIMS = os.path.join(REPO, "oracle", "shims")
_TLX_KEYS = ("tensorlayerx", "tensorlayerx.nn", "tensorlayerx.ops", "tensorlayerx.nn.initializers", "tensorlayerx.initializers")
_SHIM_KEYS = ("paddle", "paddle.regularizer", "paddle2tlx", "paddle2tlx.pd2tlx", "paddle2tlx.pd2tlx.ops", "paddle2tlx.pd2tlx.ops.tlxops",
              "paddle2tlx.pd2tlx.utils", "decorator", "torchvision", "torchvision.ops",
              # mobilenetv2.py:6-7 / mobilenetv3.py:10-11 import their siblings as TOP-LEVEL packages (`from utils.common_func
              # import ...`, `from ops.ops_fusion import ...`): they resolve with the classification directory on sys.path
              "utils", "utils.common_func", "ops", "ops.ops_fusion", "ops.theseus_layer")


def import_reference(relpath, modname, paddle=False, package=None):
    """Load one reference source file UNMODIFIED, by path, with `tensorlayerx` resolved to the oracle's torch-CPU
    stand-in (oracle/tlx_cpu).  paddle=True: the file is one of the Paddle-converted ones — `paddle`, `paddle2tlx`,
    `decorator`, `torchvision` resolve to oracle/shims/ (see its README) and the functions of the stand-in return
    PdTensor (Paddle tensor-method spellings, oracle/tlx_cpu/pd.py).  package=(name, dir): load the file as module
    `name.<stem>` of a synthetic parent package rooted at `dir`, so its relative imports resolve against the reference
    tree without running the parent's __init__ (detection/__init__.py pulls detr / ssd / ppyoloe)."""
    import oracle.tlx_cpu as tlx_cpu
    saved = {k: sys.modules.get(k) for k in _TLX_KEYS + _SHIM_KEYS}
    saved_path = list(sys.path)
    tlx = tlx_cpu
    ops = tlx_cpu.ops
    if paddle:
        ops = pd.pd_module(tlx_cpu.ops, "tensorlayerx.ops")
        tlx = pd.pd_module(tlx_cpu, "tensorlayerx", ops=ops, arange=ops.arange, stack=ops.stack)
    for k in _SHIM_KEYS:
        sys.modules.pop(k, None)
    sys.modules["tensorlayerx"] = tlx
    sys.modules["tensorlayerx.nn"] = tlx_cpu.nn
    sys.modules["tensorlayerx.ops"] = ops
    sys.modules["tensorlayerx.nn.initializers"] = tlx_cpu.nn.initializers
    sys.modules["tensorlayerx.initializers"] = tlx_cpu.nn.initializers
    sys.path.insert(0, SHIMS)
    sys.path.insert(0, os.path.join(REF, "tlxcv", "models", "classification"))
    created = []
    try:
        if package is not None:
            pname, pdir = package
            parent = types.ModuleType(pname)
            parent.__path__ = [os.path.join(REF, pdir)]
            parent.__package__ = pname
            sys.modules[pname] = parent
            created.append(pname)
            stem = os.path.splitext(os.path.basename(relpath))[0]
            mod = importlib.import_module(f"{pname}.{stem}")
            created += [k for k in sys.modules if k.startswith(pname + ".")]
            return mod
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        sys.path[:] = saved_path
        for k in created:
            sys.modules.pop(k, None)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


# The reference files by name: classification/<name>.py unless listed in _ELSEWHERE as (path under tlxcv/models, package).
_PADDLE = {"swin_transformer", "mobilenetv2", "mobilenetv3", "convnext", "cswin_transformer", "densenet", "ghostnet", "googlenet", "gvt",
           "levit", "mixnet", "pvt_v2", "res2net", "shufflenetv2", "squeezenet", "tnt", "van"}
_ELSEWHERE = {"darknet": ("detection/backbones/darknet.py", None), "mobilenet_v1": ("detection/backbones/mobilenet_v1.py", None),
              "detr": ("detection/detr.py", None), "yolov3": ("detection/yolov3.py", ("refdet", "tlxcv/models/detection")),
              "deeplab": ("segmentation/deeplab.py", ("refseg", "tlxcv/models/segmentation"))}


def reference(name):
    """The reference model file `name` (`squeezenet`, `yolov3`, `deeplab`, ...) as a module loaded by import_reference."""
    relpath, package = _ELSEWHERE.get(name, (f"classification/{name}.py", None))
    return import_reference("tlxcv/models/" + relpath, "ref_" + name, paddle=name in _PADDLE, package=package)


def restated(name):
    """A restatement module of tests/ (`cswin_restated`, ...)."""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    return importlib.import_module(name)


TAIL = "OUT restatement_max_abs_diff pinned_by param_names torch_version"
PINNED = "reference-file-on-tlx_cpu"


@dataclasses.dataclass
class Job:
    """One model fixture.  The callables take the loaded modules, so the table below holds no imported state."""
    fname: str
    ref: str                              # reference(ref) is the model file
    build: Callable                       # (reference module) -> model
    restate: Callable                     # (restatement module, params, x, peaks) -> output or outputs; may append intermediates to peaks
    image: Callable                       # (restatement module, batch, input seed) -> the input as a numpy array, channels first
    batch: int
    seeds: list                           # (weight seed, input seed) pairs, tried in order
    meta: dict                            # the fixture's leading keys, then come weight_seed, input_seed, batch and hw (unless None)
    hw: object = None
    pinned_by: str = PINNED
    restated: str = None                  # module under tests/ with the restatement; None: oracle.functional
    dtype: torch.dtype = torch.float64
    outs: tuple = ("logits",)             # names of the outputs; `logits<i>` is stored with its `argmax<i>`, None is checked but not stored
    tail: str = TAIL                      # the keys after hw, OUT standing for the outputs
    forward: Callable = lambda model, x: model(x)
    class_axis: int = -1
    margins: str = None                   # "all": every row's top-1 margin must exceed 2 x the bound; "half": half of the rows' must
    distinct: bool = False                # the rows of a batch must not share one argmax
    emulate: Callable = None              # (restatement module, fp16-rounded params, fp16-rounded x, rounding) -> fp16-emulated output
    also: tuple = ()                      # further (build, restate) pairs that must agree as well, on the accepted seeds

    def compare(self, ref, RS, build, restate, wseed, xseed):
        """Fill, run the reference forward and the restatement, require them to agree -> shapes, params, x, outputs, diff, peaks."""
        model = build(ref)
        shapes = seeded.shapes_of(model)
        params = seeded.fill(shapes, wseed)
        model.load_dict(params)
        model.set_eval()
        model.to(self.dtype)
        x = torch.from_numpy(self.image(RS, self.batch, xseed)).to(self.dtype)
        p = {k: torch.from_numpy(v).to(self.dtype) for k, v in params.items()}
        peaks = []
        with torch.no_grad():
            got = self.forward(model, pd.wrap(x) if self.ref in _PADDLE else x)
            want = restate(RS, p, x, peaks)
        got = [torch.as_tensor(pd.unwrap(o)) for o in (got if isinstance(got, (list, tuple)) else [got])]
        want = list(want) if isinstance(want, (list, tuple)) else [want]
        assert len(got) == len(want) == len(self.outs) and all(a.shape == b.shape for a, b in zip(got, want))
        d = max((a - b).abs().max().item() for a, b in zip(got, want))
        same = all(bool((a.argmax(self.class_axis) == b.argmax(self.class_axis)).all())
                   for n, a, b in zip(self.outs, got, want) if n and n.startswith("logits"))
        assert d <= 1e-5 and same, f"{self.fname}: restatement disagrees with the reference graph (max|diff| {d:.3e}, argmax equal {same})"
        return shapes, p, x, got, d, [float((t[1] if isinstance(t, tuple) else t).abs().max()) for t in peaks]

    def write(self, path):
        ref = reference(self.ref)
        RS = restated(self.restated) if self.restated else OF
        for wseed, xseed in self.seeds:
            shapes, p, x, got, d, peaks = self.compare(ref, RS, self.build, self.restate, wseed, xseed)
            emu_err = 0.0
            if self.emulate:          # the bound the GPU tests hold the engine to is max(0.3 % of the range, 3 x this error)
                rnd = lambda t: t.half().double()          # noqa: E731
                with torch.no_grad():
                    emu_err = float((self.emulate(RS, {k: rnd(v) for k, v in p.items()}, rnd(x), rnd) - got[0]).abs().max())
            line = (f"[{self.fname}] seeds ({wseed}, {xseed}): reference-file vs restatement max|diff| = {d:.3e}, params {len(shapes)}, "
                    f"{sum(int(np.prod(s)) for s in shapes.values())} values")
            if peaks:
                line += f"; intermediates peak at {min(peaks):.2f} .. {max(peaks):.2f}"
            if self.emulate:
                line += f"; fp16 emulation max|err| = {emu_err:.3e}"
            ok = not peaks or max(peaks) < 1000.0
            if self.margins:
                for n, o in zip(self.outs, got):
                    lg = o.float().numpy()
                    s = np.sort(lg, axis=1)
                    margin = s[:, -1] - s[:, -2]
                    need = 2 * max(0.003 * float(lg.max() - lg.min()), 3 * emu_err)
                    enough = int((margin > need).sum())
                    ok = ok and (enough == len(margin) if self.margins == "all" else enough * 2 >= len(margin))
                    line += f"\n    {n}: range {float(lg.max() - lg.min()):.3f}, argmax {o.argmax(-1).tolist()}, top-1 margins {margin.tolist()} (needed {need:.3e})"
            if self.distinct:
                ok = ok and (self.batch == 1 or len(set(got[0].argmax(-1).tolist())) > 1)
            print(line, flush=True)
            if ok:
                break
        assert ok, f"{self.fname}: margins ({self.margins}), peaks below 1000 and distinct argmax ({self.distinct}) hold for none of the seeds {self.seeds}"
        for build, restate in self.also:
            self.compare(ref, RS, build, restate, wseed, xseed)
        vals = dict(self.meta, weight_seed=wseed, input_seed=xseed, batch=self.batch)
        if self.hw is not None:
            vals["hw"] = self.hw
        arrays = {}
        for n, o in zip(self.outs, got):
            if n:
                arrays[n] = o.numpy().astype(np.float32)
            if n and n.startswith("logits"):
                arrays["argmax" + n[6:]] = o.argmax(self.class_axis).numpy().astype(np.int64)
        computed = dict(restatement_max_abs_diff=np.float64(d), fp16_emulated_err=np.float64(emu_err), pinned_by=self.pinned_by,
                        param_names=np.array(list(shapes.keys())), module_peaks=np.array(peaks), torch_version=torch.__version__,
                        param_shapes=np.array([",".join(str(v) for v in s) for s in shapes.values()]))
        for k in self.tail.split():
            vals.update(arrays if k == "OUT" else {k: computed[k]})
        np.savez_compressed(path, **vals)


@dataclasses.dataclass
class Special:
    """A fixture with a writer of its own."""
    fname: str
    write: Callable                       # (path of the npz)


def gen_detr_mha(path):
    """DETR's MultiHeadAttention (detection/detr.py:965-1062), the reference's own class loaded by path: a cross-attention
    case (7 queries over 13 memory tokens, batch 2, with an additive mask, weights wanted) and a self-attention case
    (197 tokens, the ViT length, no mask)."""
    ref = reference("detr")
    out = {}
    rng = np.random.default_rng(40)
    for tag, D, H, T, S, B, masked in (("cross", 64, 4, 7, 13, 2, True), ("self", 128, 4, 197, 197, 2, False)):
        m = ref.MultiHeadAttention(D, H)
        shapes = seeded.shapes_of(m)
        params = seeded.fill(shapes, 41)
        m.load_dict(params)
        m.set_eval()
        q = torch.from_numpy(rng.standard_normal((T, B, D)).astype(np.float32))
        kv = q if tag == "self" else torch.from_numpy(rng.standard_normal((S, B, D)).astype(np.float32))
        mask = None
        if masked:
            mask = torch.from_numpy(np.where(rng.random((T, S)) < 0.25, -1e9, 0.0).astype(np.float32))
            mask[:, 0] = 0.0
        with torch.no_grad():
            o, w = m((q, kv, kv), attn_mask=mask)
            o2, w2 = OF.detr_mha({k: torch.from_numpy(v) for k, v in params.items()}, "", q, kv, kv, H, mask)
        d = max((o - o2).abs().max().item(), (w - w2).abs().max().item())
        same = bool((o.reshape(-1, D).argmax(-1) == o2.reshape(-1, D).argmax(-1)).all() and (w.reshape(-1, S).argmax(-1) == w2.reshape(-1, S).argmax(-1)).all())
        print(f"[detr mha {tag}] reference-file vs restatement: max|diff| = {d:.3e}, argmax equal = {same}")
        assert d <= 1e-5 and same, f"detr mha {tag}: restatement disagrees with the reference graph"
        out.update({f"{tag}_q": q.numpy(), f"{tag}_kv": kv.numpy(), f"{tag}_out": o.numpy(), f"{tag}_weights": w.numpy(),
                    f"{tag}_dims": np.array([D, H, T, S, B]), f"{tag}_diff": np.float64(d)})
        if mask is not None:
            out[f"{tag}_mask"] = mask.numpy()
    np.savez_compressed(path, weight_seed=41, pinned_by=PINNED,
                        restatement_max_abs_diff=np.float64(max(out["cross_diff"], out["self_diff"])),
                        param_names=np.array(list(shapes.keys())), torch_version=torch.__version__, **out)


def gen_yolo_post(path):
    """YOLOv3 post-processing on the committed yolov3_b1 case: head maps from the reference's own model object;
    decode = oracle/detection.py's restatement of Paddle's yolo_box (UNPINNED: the op exists on the Paddle backend only);
    NMS = the reference's OWN tlx_multiclass_nms (detection/utils/ops.py:255-329, torchvision.ops from oracle/shims) run on
    those boxes, and required to equal the restatement.  Plus a denser synthetic NMS case (overlapping boxes, 7 classes)."""
    from oracle import detection as OD
    ref = reference("yolov3")
    ref_nms = ref.cvt_results.__globals__["tlx_multiclass_nms"]
    g = np.load(os.path.join(GOLDEN, "yolov3_b1.npz"))
    heads = [torch.from_numpy(g[f"head{i}"]) for i in range(3)]
    model = ref.YOLOv3()
    anchors = model.yolo_head.mask_anchors
    hw = int(g["hw"])
    im_shape = torch.tensor([[hw, hw]], dtype=torch.float32)
    boxes, scores = OD.yolo_decode(heads, anchors, 92, im_shape, torch.ones_like(im_shape), conf_thresh=0.005, downsample_ratio=32)
    sys.path.insert(0, SHIMS)
    try:
        out = {}
        for tag, b, s_, thr in (("yolo", boxes, scores, 0.01), ("dense", None, None, 0.3)):
            if b is None:
                rng = np.random.default_rng(50)
                ctr, wh = rng.uniform(0, 200, (2, 600, 2)), rng.uniform(5, 60, (2, 600, 2))
                b = torch.from_numpy(np.concatenate([ctr - wh / 2, ctr + wh / 2], -1).astype(np.float32))
                s_ = torch.from_numpy((rng.random((2, 600, 7)) ** 3).astype(np.float32))
            det_ref = ref_nms(b, s_, score_threshold=thr, nms_threshold=0.5, keep_top_k=100)
            det_re = OD.multiclass_nms(b, s_, thr, 0.5, 100)
            for x, y in zip(det_ref, det_re):
                assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), "NMS restatement disagrees with tlx_multiclass_nms"
            out[f"{tag}_boxes"], out[f"{tag}_scores"] = b.numpy(), s_.numpy()
            out[f"{tag}_counts"] = np.array([0 if d is None else d.shape[0] for d in det_ref], dtype=np.int32)
            out[f"{tag}_det"] = np.concatenate([np.zeros((0, 6), np.float32)] + [d.numpy() for d in det_ref if d is not None])
            out[f"{tag}_thr"] = np.float32(thr)
            print(f"[yolo post {tag}] {b.shape[1]} boxes -> detections per image {out[f'{tag}_counts'].tolist()}")
    finally:
        sys.path.remove(SHIMS)
    np.savez_compressed(path, anchors=np.array(anchors, dtype=np.float32), hw=hw,
                        pinned_by="reference-file-on-tlx_cpu (NMS: the reference's tlx_multiclass_nms with torchvision.ops from oracle/shims; "
                                  "box decode: restatement of paddle.vision.ops.yolo_box, UNPINNED — Paddle-only in the reference)",
                        restatement_max_abs_diff=np.float64(0.0), **out)


def gen_tlx_npz(path):
    """SURVEY 8f rank 1 — checkpoint interchange.  Two small instances of the reference's own classes (its
    VisionTransformer at 32 x 32 / width 32 / depth 2, its MobileNetV1 at scale 0.125, 10 classes) are filled from the
    seeded recipe on the stand-in and written with `model.save_weights(path)` (train.py:55): the positional `params`
    object array.  The fixture keeps that array, the seeds, and the reference models' logits on a seeded input, so the
    engine side can be checked to (i) restore every named weight from the positional list and (ii) compute the same
    logits from the restored weights.  The on-disk format itself is [TLX-recalled] (oracle/tlx_cpu/nn.py)."""
    out = {}
    vit = reference("vision_transformer")
    mb = reference("mobilenetv1")
    cases = (("vit", lambda: vit.VisionTransformer(img_size=32, patch_size=8, num_classes=10, embed_dim=32, depth=2, num_heads=2,
                                                   mlp_ratio=2, qkv_bias=True, epsilon=1e-6), 21, 32),
             ("mbv1", lambda: mb.MobileNetV1(scale=0.125, num_classes=10), 22, 64))
    for tag, ctor, wseed, hw in cases:
        model = ctor()
        shapes = seeded.shapes_of(model)
        model.load_dict(seeded.fill(shapes, wseed))
        model.set_eval()
        with tempfile.TemporaryDirectory() as d:
            ckpt = os.path.join(d, "model.npz")
            model.save_weights(ckpt)
            fresh = ctor()
            fresh.load_weights(ckpt)
            fresh.set_eval()
            params = np.load(ckpt, allow_pickle=True)["params"]
        x = torch.from_numpy(seeded.image_batch(2, 30, hw=hw))
        with torch.no_grad():
            y, y2 = model(x), fresh(x)
        assert torch.equal(y, y2), "stand-in save_weights -> load_weights must round-trip"
        print(f"[tlx npz {tag}] {len(params)} arrays, {sum(int(np.prod(a.shape)) for a in params)} values, logits std {y.std().item():.3f}")
        for i, a in enumerate(params):
            out[f"{tag}_params_{i:03d}"] = np.asarray(a, dtype=np.float32)
        out[f"{tag}_n"] = len(params)
        out[f"{tag}_weight_seed"], out[f"{tag}_input_seed"], out[f"{tag}_hw"] = wseed, 30, hw
        out[f"{tag}_logits"] = y.numpy().astype(np.float32)
        out[f"{tag}_param_names"] = np.array(list(shapes.keys()))
    np.savez_compressed(path, pinned_by="reference-file-on-tlx_cpu (small instances of the reference's VisionTransformer / MobileNetV1; "
                        "positional checkpoint written by the stand-in's save_weights, format [TLX-recalled])",
                        restatement_max_abs_diff=np.float64(0.0), **out)


# ---- builders and forwards that need more than one expression

def yolov3_forward(model, x):
    """YOLOv3.forward (yolov3.py:51-104) followed by hand up to the head outputs — backbone, neck, yolo_head of the reference's own
    model object — because the next line, post_process, needs `yolo_box_func`, which is None off Paddle
    (detection/utils/ops.py:436-452).  -> the three heads, then the three neck maps."""
    body = model.backbone({"images": x})
    neck = model.neck(body, model.for_mot)
    return list(model.yolo_head({"images": x, "neck_feats": neck})) + list(neck)


def yolov3_restated(OF, p, x, peaks):
    _, neck, head = OF.yolov3(p, x)
    return list(head) + list(neck)


def deeplab_model(ref, ctor, num_classes, data_format):
    """ResNet_vd keeps its blocks in a list of lists that no registry walks: registered as stage_list_{s}_{i}."""
    model = getattr(ref, ctor)(num_classes=num_classes, data_format=data_format)
    for s, stage in enumerate(model.backbone.stage_list):
        for i, blk in enumerate(stage):
            model.backbone.add_module(f"stage_list_{s}_{i}", blk)
    return model


def gvt_small(ref, cls, heads, mlp_ratios, **kw):
    return getattr(ref, cls)(img_size=112, patch_size=4, class_num=10, embed_dims=[64, 128, 256], num_heads=heads, mlp_ratios=mlp_ratios,
                             qkv_bias=True, layer_norm=partial(ref.nn.LayerNorm, epsilon=1e-6), depths=[2, 2, 2], sr_ratios=[4, 2, 1], **kw)


def levit_small96(ref):
    return ref.LeViT(img_size=96, patch_size=16, embed_dim=[64, 96, 128], key_dim=[16] * 3, depth=[1, 2, 1], num_heads=[2, 3, 4],
                     attn_ratio=[2] * 3, mlp_ratio=[2] * 3, down_ops=[['Subsample', 16, 4, 4, 2, 2], ['Subsample', 16, 6, 4, 2, 2]],
                     hybrid_backbone=ref.b16(64, ref.nn.Hardswish), class_num=10, distillation=True)


CSWIN_SMALL96 = dict(image_size=96, class_num=10, embed_dim=64, depths=[1, 2, 2, 1], splits=[1, 2, 3, 3], num_heads=[2, 4, 8, 16])


def search(s0):
    return [(s0 + i, s0 + 10 + i) for i in range(8)]


# ---- the table

def _fp32(fname, ref, build, restate, batch, wseed, xseed, meta, hw=None, **kw):
    """The fp32 fixtures on oracle.functional: one seed pair, no acceptance rule; the input is seeded.image_batch at hw (224 if None)."""
    return Job(fname + ".npz", ref, build, lambda OF, p, x, peaks: restate(p, x), lambda OF, b, s: seeded.image_batch(b, s, hw=hw or 224),
               batch, [(wseed, xseed)], meta, hw=hw, dtype=torch.float32, **kw)


def _fp64(fname, ref, rs, build, restate, batch, size, seeds, meta, pinned_by, margins="all", input=None, **kw):
    """The float64 fixtures on tests/<rs>_restated.py: the input is its <rs>_input(batch, seed, *size), `hw` is stored as (h, w)."""
    return Job(fname + ".npz", ref, build, restate, lambda RS, b, s: getattr(RS, input or rs + "_input")(b, s, *size), batch, seeds,
               dict(meta, data_format=meta.get("data_format", "channels_first")), hw=np.array(size if len(size) == 2 else size * 2), pinned_by=pinned_by,
               restated=rs + "_restated", margins=margins, **kw)


def jobs():
    P = "reference-file-on-tlx_cpu ("
    out = [
        _fp32("resnet50_b4", "resnet", lambda r: r.resnet50(), lambda p, x: OF.resnet(p, x, 50), 4, 1, 0, dict(arch="resnet50")),          # BASELINE.json configs[0]
        _fp32("resnet18_b2", "resnet", lambda r: r.resnet18(), lambda p, x: OF.resnet(p, x, 18), 2, 11, 10, dict(arch="resnet18")),
    ]
    # the two 224 x 224 ViT fixtures hold no `hw` key
    for fname, arch, batch, wseed, xseed, hw in (("vit_b16_b2", "vit_base_patch16_224", 2, 2, 0, None),          # BASELINE.json configs[2] graph
                                                 ("vit_small_b1", "vit_small_patch16_224", 1, 12, 3, None),          # no qkv bias, qk_scale override, hd=96
                                                 ("vit_b16_384_b1", "vit_base_patch16_384", 1, 21, 19, 384)):          # 577 tokens: the long-sequence attention
        out.append(_fp32(fname, "vision_transformer", lambda r, a=arch: getattr(r, a)(), lambda p, x, a=arch: OF.vit(p, x, a), batch, wseed, xseed,
                         dict(arch=arch), hw))
    pd_pinned = P + "paddle / paddle2tlx import shims, Paddle tensor-method spellings: oracle/shims, oracle/tlx_cpu/pd.py)"
    for fname, ref, ctor, fn, batch, wseed, xseed, hw in (
            ("swin_b_b2", "swin_transformer", "swintransformer_base_patch4_window7_224", None, 2, 3, 0, 224),          # BASELINE.json configs[3] graph
            ("swin_t_b1", "swin_transformer", "swintransformer_tiny_patch4_window7_224", None, 1, 13, 4, 224),
            ("swin_b_w12_384_b1", "swin_transformer", "swintransformer_base_patch4_window12_384", None, 1, 22, 20, 384),          # 144-token windows
            ("mobilenetv2_b2", "mobilenetv2", "mobilenet_v2", OF.mobilenetv2, 2, 7, 5, 128),
            ("mobilenetv3_small_b2", "mobilenetv3", "mobilenet_v3_small", lambda p, x: OF.mobilenetv3(p, x, OF.MBV3_SMALL), 2, 8, 6, 128),
            ("mobilenetv3_large_b1", "mobilenetv3", "mobilenet_v3_large", lambda p, x: OF.mobilenetv3(p, x, OF.MBV3_LARGE), 1, 9, 7, 128)):
        out.append(_fp32(fname, ref, lambda r, c=ctor: getattr(r, c)(), fn or (lambda p, x, c=ctor: OF.swin(p, x, c)), batch, wseed, xseed,
                         dict(arch=ctor), hw, pinned_by=pd_pinned))
    out += [
        _fp32("mobilenetv1_b2", "mobilenetv1", lambda r: r.MobileNetV1(), OF.mobilenetv1, 2, 4, 1, dict(arch="MobileNetV1")),
        _fp32("vgg16_b1", "vgg", lambda r: r.vgg16(batch_norm=False), lambda p, x: OF.vgg(p, x, "vgg16", False), 1, 10, 8, dict(arch="vgg16", batch_norm=False)),
        _fp32("vgg11_bn_b2", "vgg", lambda r: r.vgg11(batch_norm=True), lambda p, x: OF.vgg(p, x, "vgg11", True), 2, 11, 9, dict(arch="vgg11", batch_norm=True)),
        _fp32("alexnet_b2", "alexnet", lambda r: r.alexnet(), OF.alexnet, 2, 12, 10, dict(arch="alexnet")),
    ]
    for fname, card, batch, hw, wseed, xseed in (("resnext50_32x4d_b2", 32, 2, 96, 13, 11), ("resnext50_64x4d_b1", 64, 1, 64, 14, 12)):
        out.append(_fp32(fname, "resnext", lambda r, c=card: r.ResNeXt(layers=50, cardinality=c), lambda p, x, c=card: OF.resnext(p, x, 50, c),
                         batch, wseed, xseed, dict(layers=50, cardinality=card), hw))
    for fname, ref, arch, fn, batch, hw, wseed, xseed in (
            ("resnest50_b2", "resnest", "resnest50", OF.resnest, 2, 96, 17, 15),
            ("resnest50_fast_b1", "resnest", "resnest50_fast_1s1x64d", OF.resnest, 1, 64, 18, 16),          # radix 1 (sigmoid gate), avd_first
            ("efficientnet_b0_b2", "efficientnet", "efficientnet_b0", OF.efficientnet, 2, 224, 15, 13),
            ("efficientnet_b2_b1", "efficientnet", "efficientnet_b2", OF.efficientnet, 1, 130, 16, 14)):          # width / depth multipliers, odd extents under 'SAME'
        build = (lambda r, a=arch: r.efficientnet(a)) if ref == "efficientnet" else (lambda r, a=arch: getattr(r, a)())
        out.append(_fp32(fname, ref, build, lambda p, x, a=arch, fn=fn: fn(p, x, a), batch, wseed, xseed, dict(arch=arch), hw))
    images = lambda model, x: model({"images": x})          # noqa: E731
    det_kw = dict(feature_maps=[4, 6, 13, 14, 15], extra_block_filters=[[256, 512], [128, 256]])
    out += [
        _fp32("darknet53_b1", "darknet", lambda r: r.DarkNet(), OF.darknet53, 1, 5, 2, dict(arch="DarkNet53"), 64, forward=images, outs=("feat0", "feat1", "feat2")),
        Job("yolov3_b1.npz", "yolov3", lambda r: r.YOLOv3(), yolov3_restated, lambda OF, b, s: seeded.image_batch(b, s, hw=64), 1, [(6, 3)],
            dict(arch="YOLOv3"), hw=64, dtype=torch.float32, forward=yolov3_forward, outs=("head0", "head1", "head2", None, None, "neck2"),
            pinned_by=P + "backbone, neck, yolo_head of the reference's YOLOv3 object; decorator / torchvision from oracle/shims)"),
        # the detection MobileNet backbone with the SSD-style extra blocks switched on, so that ExtraBlock / relu6 are covered
        _fp32("mobilenet_det_b1", "mobilenet_v1", lambda r: r.MobileNet(with_extra_blocks=True, **det_kw), lambda p, x: OF.mobilenet_det(p, x, **det_kw),
              1, 23, 17, dict(arch="MobileNet(det)"), 128, forward=images, outs=tuple(f"feat{i}" for i in range(5))),
        Special("tlx_npz_small.npz", gen_tlx_npz), Special("detr_mha.npz", gen_detr_mha), Special("yolov3_post_b1.npz", gen_yolo_post),
    ]

    for nc, batch, size, wseed, xseed, fname in ((1000, 2, (224, 224), 11, 21, "convnext_tiny_b2"), (10, 1, (96, 160), 12, 22, "convnext_c10_96x160_b1")):
        out.append(_fp64(fname, "convnext", "convnext", lambda r, nc=nc: r.convnext(class_num=nc), lambda RS, p, x, peaks: RS.convnext(p, x), batch, size,
                         [(wseed, xseed)], dict(arch="convnext", class_num=nc), margins="half", pinned_by=P + "classification/convnext.py unmodified; "
                         "tlx_GELU, tlx_linspace, tlx_get_tensor_shape, ops.sqrt and Parameter.set_value supplied at run time)"))
    for arch, build, cfg, nc, batch, hw in (("cswin_tiny", lambda r: r.CSwintransformer_thiny(class_num=1000), "TINY", 1000, 2, 224),
                                            ("cswin_c10_96", lambda r: r.CSwinTransformer(**CSWIN_SMALL96), "SMALL96", 10, 1, 96)):
        out.append(_fp64(f"{arch}_b{batch}", "cswin_transformer", "cswin", build,
                         lambda RS, p, x, peaks, cfg=cfg: RS.cswin(p, x, cfg=getattr(RS, cfg), stage_inputs=peaks), batch, (hw,), search(16),
                         dict(arch=arch, num_classes=nc), P + "classification/cswin_transformer.py unmodified; random_normal, Linear.b_init, tlx_GELU, "
                         "tlx_linspace, ops.matmul, convert_to_tensor(dtype string) and PdTensor.flatten / .chunk supplied at run time)"))
    for nc, batch, size, wseed, xseed, fname in ((1000, 2, (224, 224), 13, 23, "densenet121_b2"), (10, 1, (96, 160), 14, 24, "densenet121_c10_96x160_b1")):
        out.append(_fp64(fname, "densenet", "densenet", lambda r, nc=nc: r.densenet121(num_classes=nc), lambda RS, p, x, peaks: RS.densenet(p, x, 121, peaks),
                         batch, size, [(wseed, xseed)], dict(arch="densenet121", num_classes=nc), margins="half", pinned_by=P + "classification/densenet.py "
                         "unmodified; Module.add_sublayer, tlx_MaxPool2d, tlx_AvgPool2d and a 1-D xavier_uniform supplied at run time)"))
    for arch, scale, nc, batch, size, s0, fname in (("ghostnet_x1_0", 1.0, 1000, 2, (224, 224), 31, "ghostnet_x1_0_b2"),
                                                    ("ghostnet_x0_5", 0.5, 10, 1, (96, 160), 32, "ghostnet_x0_5_c10_96x160_b1"),
                                                    ("ghostnet_x1_3", 1.3, 10, 1, (96, 160), 33, "ghostnet_x1_3_c10_96x160_b1")):
        out.append(_fp64(fname, "ghostnet", "ghostnet", lambda r, a=arch, nc=nc: getattr(r, a)(class_num=nc),
                         lambda RS, p, x, peaks, sc=scale: RS.ghostnet(p, x, sc, peaks), batch, size, search(s0), dict(arch=arch, num_classes=nc),
                         P + "classification/ghostnet.py unmodified; paddle.regularizer.L2Decay, initializers.HeNormal / random_uniform, "
                         "Module.add_sublayer, tensorlayerx.ops.squeeze / clip_by_value / multiply and a list axis for tensorlayerx.expand_dims supplied at run time)"))
    for nc, pool, batch, size, s0, fname in ((1000, True, 2, (224, 224), 81, "googlenet_b2"), (10, True, 1, (200, 232), 82, "googlenet_c10_200x232_b1"),
                                             (0, False, 1, (72, 104), 83, "googlenet_maps_72x104_b1")):
        # the main head and the two aux heads; without classes the three maps instead
        out.append(_fp64(fname, "googlenet", "googlenet", lambda r, nc=nc, pool=pool: r.GoogLeNet(num_classes=nc, with_pool=pool),
                         lambda RS, p, x, peaks, nc=nc, pool=pool: RS.googlenet(p, x, nc, pool, peaks), batch, size, search(s0),
                         dict(arch="googlenet", num_classes=nc, with_pool=pool), P + "classification/googlenet.py unmodified; tlx_MaxPool2d, tlx_AvgPool2d and "
                         "tensorlayerx.ops.squeeze supplied at run time)", margins="all" if nc else None, distinct=nc > 0,
                         outs=("logits", "logits1", "logits2") if nc else ("map0", "map1", "map2"),
                         tail="restatement_max_abs_diff pinned_by param_names param_shapes module_peaks torch_version OUT"))
    gvt_pinned = P + ("classification/gvt.py unmodified; paddle.regularizer.L2Decay, initializers.random_normal, nn.ParameterList, tlxops.tlx_linspace, "
                      "paddle.matmul and tensorlayerx.ops.matmul supplied at run time)")
    for arch, fname, build, cfg, nc, batch, hw in (
            ("alt_gvt_small", "gvt_alt_small_b2", lambda r: r.alt_gvt_small(class_num=1000), "ALT_SMALL", 1000, 2, 224),
            ("pcpvt_small", "gvt_pcpvt_small_b2", lambda r: r.pcpvt_small(class_num=1000), "PCPVT_SMALL", 1000, 2, 224),
            ("gvt_alt_c10_112", "gvt_alt_c10_112_b1", lambda r: gvt_small(r, "ALTGVT", [2, 4, 8], [4, 4, 4], wss=[7, 7, 7]), "ALT_C10_112", 10, 1, 112),
            ("gvt_pcpvt_c10_112", "gvt_pcpvt_c10_112_b1", lambda r: gvt_small(r, "CPVTV2", [1, 2, 4], [8, 8, 4]), "PCPVT_C10_112", 10, 1, 112)):
        out.append(_fp64(fname, "gvt", "gvt", build, lambda RS, p, x, peaks, cfg=cfg: RS.gvt(p, x, getattr(RS, cfg), stream=peaks), batch, (hw,), search(17),
                         dict(arch=arch, num_classes=nc), gvt_pinned))
    for arch, build, cfg, nc, batch, hw in (("levit_128s", lambda r: r.levit_128s(class_num=1000), "S128", 1000, 2, 224),
                                            ("levit_c10_96", levit_small96, "SMALL96", 10, 1, 96)):
        out.append(_fp64(f"{arch}_b{batch}", "levit", "levit", build, lambda RS, p, x, peaks, cfg=cfg: RS.levit(p, x, cfg=getattr(RS, cfg), stream=peaks),
                         batch, (hw,), search(16), dict(arch=arch, num_classes=nc),
                         P + "classification/levit.py unmodified; random_normal, paddle.regularizer.L2Decay, BatchNorm1d, "
                         "Sequential.add_sublayer / _sub_layers, tensorlayerx.gather / constant, ops.matmul / ops.split, convert_to_tensor(dtype string), "
                         "paddle.matmul / transpose and PdTensor.flatten / .reshape(0 extent) supplied at run time)"))
    for arch, nc, batch, size, s0, fname in (("mixnet_s", 1000, 2, (224, 224), 51, "mixnet_s_b2"), ("mixnet_m", 10, 1, (200, 224), 52, "mixnet_m_c10_200x224_b1"),
                                             ("mixnet_l", 10, 1, (208, 200), 53, "mixnet_l_c10_208x200_b1")):
        out.append(_fp64(fname, "mixnet", "mixnet", lambda r, a=arch, nc=nc: getattr(r, a)(class_num=nc), lambda RS, p, x, peaks, a=arch: RS.mixnet(p, x, a, peaks),
                         batch, size, search(s0), dict(arch=arch, num_classes=nc), P + "classification/mixnet.py unmodified; Module.add_sublayer, "
                         "Module._sub_layers, nn.Swish, tensorlayerx.ops.split and tlx_AvgPool2d supplied at run time)", distinct=True))
    for nc, batch, size, wseed, xseed, fname in ((1000, 2, (224, 224), 15, 25, "pvt_v2_b0_b2"), (10, 1, (96, 160), 18, 28, "pvt_v2_b0_c10_96x160_b1")):
        pair = lambda lin, nc=nc: (lambda r: r.pvt_v2(class_num=nc, linear=lin),          # noqa: E731
                                   lambda RS, p, x, peaks: RS.pvt_v2(p, x, linear=lin, stage_inputs=peaks))
        out.append(_fp64(fname, "pvt_v2", "pvt_v2", *pair(False), batch, size, [(wseed, xseed)], dict(arch="pvt_v2_b0", num_classes=nc),
                         P + "classification/pvt_v2.py unmodified; tlx_linspace and tlx_GELU supplied at run time)", also=(pair(True),)))
    for layers, scales, width, nc, batch, size, s0, tag in ((50, 4, 26, 1000, 2, (224, 224), 71, "b2"), (50, 4, 26, 10, 1, (200, 232), 72, "c10_200x232_b1"),
                                                            (50, 8, 14, 10, 1, (72, 104), 73, "c10_72x104_b1")):
        arch = f"res2net{layers}_{width}w_{scales}s"
        out.append(_fp64(f"{arch}_{tag}", "res2net", "res2net", lambda r, k=dict(layers=layers, scales=scales, width=width, class_num=nc): r.Res2Net(**k),
                         lambda RS, p, x, peaks, l=layers, s=scales: RS.res2net(p, x, l, s, peaks), batch, size, search(s0),
                         dict(arch=arch, layers=layers, scales=scales, width=width, num_classes=nc), P + "classification/res2net.py unmodified; "
                         "Module.add_sublayer, tensorlayerx.ops.split, tlx_MaxPool2d and tlx_AvgPool2d supplied at run time)", distinct=True,
                         tail="OUT restatement_max_abs_diff pinned_by param_names param_shapes torch_version"))
    for rs, nc, batch, size, data_format, wseed, xseed, fname in (
            ("deeplabv3", 19, 2, (64, 64), "channels_first", 7, 17, "deeplabv3_b2"), ("deeplabv3", 2, 1, (128, 160), "channels_last", 8, 18, "deeplabv3_c2_128x160_b1"),
            ("deeplabv3p", 19, 2, (64, 64), "channels_first", 9, 19, "deeplabv3p_b2"), ("deeplabv3p", 2, 1, (128, 160), "channels_last", 10, 20, "deeplabv3p_c2_128x160_b1")):
        # fp64: a deep fp32 CPU run alone differs from the restatement by ~1e-5 in summation order
        nhwc = lambda model, x: model(x.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)          # noqa: E731
        out.append(_fp64(fname, "deeplab", "deeplab" if rs == "deeplabv3" else rs, lambda r, a=(rs, nc, data_format): deeplab_model(r, *a),
                         lambda RS, p, x, peaks, rs=rs: getattr(RS, rs)(p, x), batch, size, [(wseed, xseed)], dict(arch=rs, num_classes=nc, data_format=data_format),
                         P + "segmentation/deeplab.py unmodified" + (", deeplabv3p" if rs == "deeplabv3p" else "") + "; tlx.Resize and nn.layers.activation supplied "
                         "at run time; stage_list blocks registered as stage_list_{s}_{i})", margins=None, class_axis=1, input="seg_input",
                         **({} if data_format == "channels_first" else dict(forward=nhwc))))
    for arch, act, nc, batch, size, s0, fname in (("shufflenet_v2_x1_0", "relu", 1000, 2, (224, 224), 17, "shufflenet_v2_x1_0_b2"),
                                                  ("shufflenet_v2_swish", "swish", 10, 1, (96, 160), 18, "shufflenet_v2_swish_c10_96x160_b1"),
                                                  ("shufflenet_v2_x0_5", "relu", 10, 1, (96, 160), 19, "shufflenet_v2_x0_5_c10_96x160_b1")):
        out.append(_fp64(fname, "shufflenetv2", "shufflenet", lambda r, a=arch, nc=nc: getattr(r, a)(num_classes=nc),
                         lambda RS, p, x, peaks, act=act: RS.shufflenet(p, x, act, peaks), batch, size, search(s0), dict(arch=arch, num_classes=nc),
                         P + "classification/shufflenetv2.py unmodified; nn.Swish, Module.add_sublayer, tlxops.tlx_MaxPool2d and tensorlayerx.ops.split supplied at run time)"))
    for ver, nc, pool, batch, size, s0, fname in (("1.0", 1000, True, 2, (224, 224), 91, "squeezenet1_0_b2"), ("1.1", 1000, True, 2, (224, 224), 94, "squeezenet1_1_b2"),
                                                  ("1.1", 10, True, 1, (200, 232), 95, "squeezenet1_1_c10_200x232_b1"),
                                                  ("1.1", 0, False, 1, (72, 104), 96, "squeezenet1_1_maps_72x104_b1")):
        # the zero-mean filters of the seeded rule cancel, so fp16 storage alone costs about 0.3 % of this model's logit range: the
        # restatement runs once more with input, weights and every conv output rounded to fp16, and its error is stored for the bound
        logits = nc > 0 and pool
        out.append(_fp64(fname, "squeezenet", "squeezenet", lambda r, a=(ver, nc, pool): r.SqueezeNet(a[0], num_classes=a[1], with_pool=a[2]),
                         lambda RS, p, x, peaks, a=(ver, nc, pool): RS.squeezenet(p, x, *a, peaks), batch, size, search(s0),
                         dict(arch="squeezenet", version=ver, num_classes=nc, with_pool=pool), P + "classification/squeezenet.py unmodified; tlx_MaxPool2d and "
                         "tensorlayerx.ops.squeeze supplied at run time)", margins="all" if logits else None, distinct=logits, outs=("logits",) if logits else ("map0",),
                         emulate=lambda RS, p, x, rnd, a=(ver, nc, pool): RS.squeezenet(p, x, *a, None, rnd),
                         tail="restatement_max_abs_diff fp16_emulated_err pinned_by param_names param_shapes module_peaks torch_version OUT"))
    for arch, build, cfg, nc, batch, hw in (("tnt_small", lambda r: r.tnt_small(class_num=1000), "SMALL224", 1000, 2, 224),
                                            ("tnt_c10_64", lambda r: r.TNT(img_size=64, patch_size=16, embed_dim=128, in_dim=24, depth=2, num_heads=2, in_num_head=4,
                                                                           class_num=10), "C10_64", 10, 1, 64)):
        out.append(_fp64(f"{arch}_b{batch}", "tnt", "tnt", build, lambda RS, p, x, peaks, cfg=cfg: RS.tnt(p, x, cfg=getattr(RS, cfg), stream=peaks), batch, (hw,),
                         search(16), dict(arch=arch, num_classes=nc), P + "classification/tnt.py unmodified; paddle.nn.functional.unfold, paddle.matmul, "
                         "tensorlayerx.ops.matmul and tlxops.tlx_get_tensor_shape supplied at run time)"))
    for nc, batch, size, s0, fname in ((1000, 2, (224, 224), 16, "van_b0_b2"), (10, 1, (96, 160), 19, "van_b0_c10_96x160_b1")):
        out.append(_fp64(fname, "van", "van", lambda r, nc=nc: r.van(class_num=nc), lambda RS, p, x, peaks: RS.van(p, x, stage_inputs=peaks), batch, size, search(s0),
                         dict(arch="van_b0", num_classes=nc), P + "classification/van.py unmodified; tlx_linspace and tlx_GELU supplied at run time)"))
    return out


def differences(path, committed):
    """What makes the npz at `path` differ from the committed one: key set and order, dtype, shape, values -> a list of reasons."""
    if not os.path.isfile(committed):
        return ["no committed fixture"]
    a, b = np.load(path, allow_pickle=True), np.load(committed, allow_pickle=True)
    if a.files != b.files:
        return [f"keys {a.files} against the committed {b.files}"]
    why = []
    for k in a.files:
        u, v = a[k], b[k]
        if u.dtype != v.dtype or u.shape != v.shape:
            why.append(f"{k}: {u.dtype}{u.shape} against the committed {v.dtype}{v.shape}")
        elif not (all(np.array_equal(s, t) for s, t in zip(u, v)) if u.dtype == object else np.array_equal(u, v)):
            why.append(f"{k}: values differ")
    return why


def main(argv, todo=None):
    check = "--check" in argv
    words = [a for a in argv if a != "--check"]
    todo = jobs() if todo is None else todo
    if words:          # in the order of the words
        todo = list({j.fname: j for w in words for j in todo if w in j.fname}.values())
    torch.set_num_threads(8)
    bad, t0 = 0, time.time()
    with tempfile.TemporaryDirectory() as tmp:
        out = tmp if check else GOLDEN
        os.makedirs(out, exist_ok=True)
        for job in todo:
            t = time.time()
            torch.manual_seed(0)          # before every job: no result depends on the jobs before it
            path = os.path.join(out, job.fname)
            job.write(path)
            line = f"{job.fname}: written in {time.time() - t:.1f} s"
            if check:
                g = np.load(path)
                why = differences(path, os.path.join(GOLDEN, job.fname))
                bad += bool(why)
                seeds = f"seeds ({int(g['weight_seed'])}, {int(g['input_seed'])}), " if "input_seed" in g.files else ""
                line = f"{job.fname}: {seeds}{time.time() - t:.1f} s, " + ("equal to the committed fixture" if not why else "DIFFERENT: " + "; ".join(why))
            print(line, flush=True)
    print(f"{len(todo)} fixtures in {time.time() - t0:.1f} s" + (f", {bad} differ from the committed ones" if check else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
