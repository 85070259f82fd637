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
from tlxcv_amd import engine as E, seeded, models  # noqa: E402
from tlxcv_amd.graph import GraphedForward  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5

SHAPES = [("x0_5 stage 2", 28, 48), ("x0_5 stage 3", 14, 96), ("x0_5 stage 4", 7, 192),
          ("x1_0 stage 2", 28, 116), ("x1_0 stage 3", 14, 232), ("x1_0 stage 4", 7, 464)]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us


def ab(arms):
    """arms: {name: (fn, calls per graph, replays per round)} -> {name: (median us per call, min, max)}."""
    graphs = {}
    for k, (f, calls, _) in arms.items():
        for _ in range(2):
            f()
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for _ in range(calls):
                f()
        graphs[k].replay()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, (_, calls, replays) in arms.items():
            t[k].append(timed(graphs[k].replay, replays) / calls)
    res = {}
    for k in arms:
        v = sorted(t[k])
        res[k] = (v[len(v) // 2], v[0], v[-1])
    return res


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
        res = ab(arms)
        nbytes = 2 * batch * hw * hw * c * 2
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy = ab({"copy": (lambda: dst.copy_(src), 10, 5)})["copy"]
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
    for name, seed in (("shufflenet_v2_x0_5", 19), ("shufflenet_v2_x1_0", 17)):
        m = getattr(models, name)()
        m.load_dict(seeded.fill(seeded.shapes_of(m), seed))
        m = m.to(dev).set_eval()
        x = torch.from_numpy(seeded.image_batch(16, 0)).to(dev).repeat(batch // 16, 1, 1, 1).contiguous()
        graphs = {}
        for on in (True, False):
            E.set_option("shuffle_unit", on)
            with torch.no_grad():
                graphs[on] = GraphedForward(m, x)
        E.set_option("shuffle_unit", True)
        t = {True: [], False: []}
        for _ in range(reps):
            for on in (True, False):
                t[on].append(timed(lambda: graphs[on](), 5))
        print(f"# {name} batch {batch}, 224 x 224, fp16, hipGraph replay; median of {reps} alternated rounds of 5 forwards (min..max)")
        for on in (True, False):
            v = sorted(t[on])
            med = v[len(v) // 2]
            print(f"shuffle_unit {'on ' if on else 'off'}: {med / 1e3:8.3f} ms ({v[0] / 1e3:.3f}..{v[-1] / 1e3:.3f})  {batch / med * 1e6:8.0f} img/s", flush=True)
        d = (graphs[True].static_out.float() - graphs[False].static_out.float()).abs().max().item()
        print(f"max|logit difference| on vs off: {d:.3e}")
        del graphs, m


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "unit,model"
    if "unit" in what:
        unit()
    if "model" in what:
        model()
