"""GhostNet measurements on one MI355X (fp16).
  module: one Ghost module at every distinct module shape of ghostnet_x0_5 and ghostnet_x1_0 at 224 x 224 (ghost_module_1: ReLU, no shortcut;
          ghost_module_2: no activation, + the shortcut) on seeded maps and trained-like seeded parameters, two arms alternated:
            fused     tlxmi_ghost_module
            layers    what the fused launch replaces, the option-off arm of the same build: tlxmi_conv2d -> tlxmi_dwconv2d (-> tlxmi_affine_act
                      for the shortcut) (+ the copies of both halves where m is no whole number of 16-byte chunks)
          `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue.  Beside it the byte floor: every
          pixel's Cin channels (and the shortcut's 2 m) read once and its 2 m channels written once, at the copy bandwidth measured here by
          a device-to-device copy of the same number of bytes (read + write counted).  The fused arm keeps a shape only if its slowest
          round is faster than the layers arm's fastest one.  The times are hipGraph replay times between two events, NOT the engine
          probe's per-launch records.
          Both arms are forced (fused=True / False); the line also names the engine's default route (engine.ghost_module_supported).
  model:  ghostnet_x0_5 and ghostnet_x1_0 img/s as a hipGraph replay (graph.GraphedForward) with "ghost_module" on (the default route: fused
          where the table keeps the shape) and off, alternated.
usage: python tools/ghostnet_bench.py [batch=256] [reps=5] [module,model]"""
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


def module_shapes(name):
    """-> ordered {(hw, Cin, m, second): "blocks"}: the distinct Ghost module shapes of a variant at 224 x 224."""
    net = getattr(models, name)()
    hw, out = 112, {}
    for i, b in enumerate(net.ghost_bottleneck_list):
        g1, g2 = b.ghost_module_1, b.ghost_module_2
        out.setdefault((hw, g1.in_channels, g1.out_channels // 2, False), []).append(f"{i}.1")
        if b._stride == 2:
            hw //= 2
        out.setdefault((hw, g2.in_channels, g2.out_channels // 2, True), []).append(f"{i}.2")
    return out


def module():
    print(f"# one Ghost module, batch {batch}, fp16; us per call (hipGraph replay; median of {reps} alternated rounds, min..max)")
    for name in ("ghostnet_x0_5", "ghostnet_x1_0"):
        for (hw, cin, m, second), blocks in module_shapes(name).items():
            act = E.ACT_NONE if second else E.ACT_RELU
            g = torch.Generator().manual_seed(hw + cin + m)
            r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
            bn = lambda: ((torch.rand(m, generator=g) * 0.4 + 0.8).to(dev), (r(m) * 0.05).to(dev))      # noqa: E731
            params = E.GhostModuleParams((r(m, cin, 1, 1) * (2.0 / cin) ** 0.5).to(dev), bn(), (r(m, 1, 3, 3) * (2.0 / 9) ** 0.5).to(dev), bn(),
                                         torch.float16)
            nb = 16 if hw <= 56 else 4

            def pitched(c):
                t = torch.zeros(nb, hw, hw, E.shuffle_pitch(c))
                t[..., :c] = r(nb, hw, hw, c)
                return t.half().to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
            x = pitched(cin)
            res = pitched(2 * m) if second else None
            y = torch.empty((batch, hw, hw, E.shuffle_pitch(2 * m)), dtype=torch.float16, device=dev)
            assert E.ghost_module_takes(x, cin, m, act, y.shape[-1], res.shape[-1] if second else 0)
            routed = E.ghost_module_supported(x, cin, m, act, y.shape[-1], res.shape[-1] if second else 0)
            y_f = E.ghost_module(x, params, act, res=res, fused=True).clone()
            y_l = E.ghost_module(x, params, act, res=res, fused=False)
            d = (y_f.float() - y_l.float()).abs().max().item()
            del y_f, y_l
            calls = 10 if hw <= 56 else 4
            out = ab({"fused": (lambda: E.ghost_module(x, params, act, res=res, fused=True, out=y), calls, 5),
                      "layers": (lambda: E.ghost_module(x, params, act, res=res, fused=False, out=y), calls, 5)}, reps)
            nbytes = batch * hw * hw * (cin + 2 * m * (2 if second else 1)) * 2
            nbytes -= nbytes % 32
            copy = copy_floor(nbytes, calls, reps)
            bw = nbytes / copy[0] / 1e3                                             # GB/s: nbytes / 2 read + nbytes / 2 written
            print(f"## {name[9:]} {'ghost_module_2' if second else 'ghost_module_1'} of blocks {', '.join(b[:-2] for b in blocks)}: ({batch}, {hw}, {hw}), "
                  f"Cin = {cin}, m = {m}{', + shortcut' if second else ', ReLU'}")
            for k, (med, lo, hi) in out.items():
                print(f"{k:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  {nbytes / med / 1e3:7.1f} GB/s of the floor's bytes  = {med / copy[0]:.2f} x the byte floor", flush=True)
            print(f"byte floor: {nbytes / 1e6:.1f} MB at the measured copy bandwidth of {bw:.0f} GB/s ({copy[0]:.1f} us for the same bytes, "
                  f"{copy[1]:.1f}..{copy[2]:.1f})")
            keeps = out["fused"][2] < out["layers"][1]
            print(f"max|fused - layers| on the seeded maps: {d:.3e}; fused / layers = {out['fused'][0] / out['layers'][0]:.4f}: "
                  f"{'the fused arm is faster beyond the spread' if keeps else 'NOT faster beyond the spread: route this shape to the layers'}; "
                  f"the engine's default route here: {'fused' if routed else 'layers'}", flush=True)
            del x, res, y


def model():
    model_on_off("ghost_module", [(n, getattr(models, n), s) for n, s in (("ghostnet_x0_5", 32), ("ghostnet_x1_0", 31))], batch, reps)


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "module,model"
    if "module" in what:
        module()
    if "model" in what:
        model()
