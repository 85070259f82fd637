"""ShuffleNetV2 measurements on one MI355X (fp16).
  unit:   one stride-1 unit at every stage shape of shufflenet_v2_x0_5 and shufflenet_v2_x1_0 (batch x 28 x 28 x 48 / 116, 14 x 14 x 96 / 232,
          7 x 7 x 192 / 464) on seeded maps and trained-like seeded parameters, two arms alternated:
            fused     tlxmi_shuffle_unit (where the library takes the half width)
            layers    what the fused launch replaces, the option-off arm of the same build: tlxmi_conv2d -> tlxmi_dwconv2d -> tlxmi_conv2d ->
                      tlxmi_shuffle_concat (+ the copy of the branch half where it is not 16-byte aligned)
          `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue.  Beside it the byte floor: every
          pixel's c channels read once and written once, at the copy bandwidth measured here by a device-to-device copy of the same number of
          bytes (read + write counted).  The fused arm keeps a shape only if its slowest round is faster than the layers arm's fastest one.
          The times are hipGraph replay times between two events, NOT the engine probe's per-launch records.
  model:  shufflenet_v2_x0_5 and shufflenet_v2_x1_0 img/s as a hipGraph replay (graph.GraphedForward) with "shuffle_unit" on and off, alternated.
usage: python tools/shufflenet_bench.py [batch=256] [reps=5] [unit,model]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, models  # noqa: E402
from tools.ab import ab, copy_floor, model_on_off  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5

SHAPES = [("x0_5 stage 2", 28, 48), ("x0_5 stage 3", 14, 96), ("x0_5 stage 4", 7, 192),
          ("x1_0 stage 2", 28, 116), ("x1_0 stage 3", 14, 232), ("x1_0 stage 4", 7, 464)]


def unit():
    print(f"# one stride-1 unit, batch {batch}, fp16, ReLU; us per call (hipGraph replay; median of {reps} alternated rounds, min..max)")
    for name, hw, c in SHAPES:
        h = c // 2
        g = torch.Generator().manual_seed(hw + c)
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        bn = lambda: ((torch.rand(h, generator=g) * 0.4 + 0.8).to(dev), (r(h) * 0.05).to(dev))      # noqa: E731
        params = E.ShuffleUnitParams((r(h, h, 1, 1) * (2.0 / h) ** 0.5).to(dev), bn(), (r(h, 1, 3, 3) * (2.0 / 9) ** 0.5).to(dev), bn(),
                                     (r(h, h, 1, 1) * (2.0 / h) ** 0.5).to(dev), bn(), torch.float16)
        pitch = E.shuffle_pitch(c)
        x = torch.zeros(16, hw, hw, pitch)
        x[..., :c] = r(16, hw, hw, c)
        x = x.half().to(dev).repeat(batch // 16, 1, 1, 1).contiguous()
        y = torch.empty_like(x)
        takes = E.shuffle_unit_supported(x, c, E.ACT_RELU, pitch)
        arms = {"layers": (lambda: E.shuffle_unit(x, params, E.ACT_RELU, fused=False, out=y), 10, 5)}
        d = float("nan")
        if takes:
            y_f = E.shuffle_unit(x, params, E.ACT_RELU, fused=True).clone()
            y_l = E.shuffle_unit(x, params, E.ACT_RELU, fused=False)
            d = (y_f.float() - y_l.float()).abs().max().item()
            arms = dict({"fused": (lambda: E.shuffle_unit(x, params, E.ACT_RELU, fused=True, out=y), 10, 5)}, **arms)
        res = ab(arms, reps)
        nbytes = 2 * batch * hw * hw * c * 2
        copy = copy_floor(nbytes, 10, reps)
        bw = nbytes / copy[0] / 1e3                                             # GB/s: nbytes / 2 read + nbytes / 2 written
        print(f"## {name}: ({batch}, {hw}, {hw}, {c}), h = {h}")
        for k, (med, lo, hi) in res.items():
            print(f"{k:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  {nbytes / med / 1e3:7.1f} GB/s of read c + write c  = {med / copy[0]:.2f} x the byte floor", flush=True)
        print(f"byte floor: {nbytes / 1e6:.1f} MB at the measured copy bandwidth of {bw:.0f} GB/s ({copy[0]:.1f} us for the same bytes, "
              f"{copy[1]:.1f}..{copy[2]:.1f})")
        if takes:
            keeps = res["fused"][2] < res["layers"][1]
            print(f"max|fused - layers| on the seeded maps: {d:.3e}; fused / layers = {res['fused'][0] / res['layers'][0]:.4f}: "
                  f"{'the fused arm is faster beyond the spread' if keeps else 'NOT faster beyond the spread: route this shape to the layers'}", flush=True)
        else:
            print("the library does not take this half width: the layers arm is the route", flush=True)


def model():
    model_on_off("shuffle_unit", [(n, getattr(models, n), s) for n, s in (("shufflenet_v2_x0_5", 19), ("shufflenet_v2_x1_0", 17))], batch, reps)


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "unit,model"
    if "unit" in what:
        unit()
    if "model" in what:
        model()
