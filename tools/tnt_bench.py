"""TNT-S measurements on one MI355X (fp16).
  kernel: the inner launch at tnt_small's shape (batch x 196 patches of 16 pixels x 24 channels; 50 176 patches at batch 256) on seeded
          rows and trained-like seeded parameters, the pixel map updated in place and y_norm written, as the model calls it, with the
          fused arm (tlxmi_tnt_inner) and the plain arm (tlxmi_tnt_inner_plain) forced, alternated: `calls` calls of an arm as one hipGraph
          (10 for the fused arm, 2 for the plain one, which is not tuned), so the replay times kernels and not the host's enqueue.  Beside
          it the byte floor: x read once, y and y_norm written once (3 x patches x 16 x 24 fp16 values), at the copy bandwidth measured
          here by a device-to-device copy of a buffer of the same three-map size (read + write counted).  The fused arm keeps the shape
          only if its slowest round is faster than the plain arm's fastest one.
          The times are hipGraph replay times between two events, NOT the engine probe's per-launch records.
  model:  tnt_small img/s as a hipGraph replay (graph.GraphedForward) with "tnt_inner" on and off, alternated.
usage: python tools/tnt_bench.py [batch=256] [reps=5] [kernel,model]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, seeded, models  # noqa: E402
from tools.ab import ab, copy_floor, model_on_off  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def kernel():
    patches = batch * 196
    print(f"# the inner launch of tnt_small, batch {batch}: {patches} patches of 16 x 24, fp16; us per call (hipGraph replay; median of {reps} "
          "alternated rounds, min..max)")
    m = models.tnt_small()
    m.load_dict(seeded.fill(seeded.shapes_of(m), 16))
    m = m.to(dev).set_eval()
    packed = m.blocks[0].inner_packed()
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(patches, 16, 24, generator=g).half().to(dev)
    ref = {k: E.tnt_inner(x0, packed, 4, fused=k) for k in (True, False)}
    dy = (ref[True][0].float() - ref[False][0].float()).abs().max().item()
    dn = (ref[True][1].float() - ref[False][1].float()).abs().max().item()
    # in place, as the model runs it: the values drift from call to call, the work does not (no data-dependent branch in either arm);
    # LayerNorm keeps the rows O(1)
    x = x0.clone()
    run = lambda fused: E.tnt_inner(x, packed, 4, fused=fused, out=x)      # noqa: E731
    res = ab({"fused": (lambda: run(True), 10, 5), "plain": (lambda: run(False), 2, 2)}, reps)
    assert torch.isfinite(x).all()
    nbytes = 3 * patches * 16 * 24 * 2
    copy = copy_floor(nbytes, 10, reps)
    bw = nbytes / copy[0] / 1e3                                             # GB/s: nbytes / 2 read + nbytes / 2 written
    for k, (med, lo, hi) in res.items():
        print(f"{k:5s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  {nbytes / med / 1e3:7.1f} GB/s of x + y + y_norm", flush=True)
    print(f"byte floor: {nbytes / 1e6:.1f} MB at the measured copy bandwidth of {bw:.0f} GB/s ({copy[0]:.1f} us for the same bytes, "
          f"{copy[1]:.1f}..{copy[2]:.1f}); fused / floor = {res['fused'][0] / copy[0]:.2f}")
    keeps = res["fused"][2] < res["plain"][1]
    print(f"max|fused - plain| on the seeded rows: y {dy:.3e}, y_norm {dn:.3e}; fused / plain = {res['fused'][0] / res['plain'][0]:.4f}: "
          f"{'the fused arm is faster beyond the spread' if keeps else 'NOT faster beyond the spread: route this shape to the plain arm'}", flush=True)


def model():
    model_on_off("tnt_inner", [("tnt_small", models.tnt_small, 16)], batch, reps, forwards=(10, 3))


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "kernel,model"
    if "kernel" in what:
        kernel()
    if "model" in what:
        model()
