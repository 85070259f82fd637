"""SqueezeNet measurements on one MI355X (fp16).
  shape: each of the eight Fire modules of both versions at 224 x 224 sizes (twelve distinct shapes), on seeded maps and seeded filters,
         two arms alternated:
            fused     tlxmi_fire_module
            layered   what the launch replaces, the option-off arm of the same build: tlxmi_conv2d x 3 with bias + ReLU epilogues
         `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue.  Beside it the byte floor: one
         read of x and one write of y at 8 TB/s (the nominal HBM bandwidth; a device-to-device copy of the same bytes is timed next to
         it).  The fused arm wins a shape only if its slowest round is faster than the layered arm's fastest one.  The times are hipGraph
         replay times between two events, NOT the engine probe's per-launch records.  Only a shape the fused arm wins belongs in
         engine.FIRE_MODULE_WINS.
  model: SqueezeNet 1.0 and 1.1 img/s as a hipGraph replay (graph.GraphedForward), three arms alternated: every module forced onto the
         launch, the default route (the measured table) and "fire_module" off.
usage: python tools/squeezenet_bench.py [batch=256] [reps=5] [shape,model]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, seeded, models  # noqa: E402
from tlxcv_amd.graph import GraphedForward  # noqa: E402
from tools.ab import ab, copy_floor, timed  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
HBM = 8.0e12        # bytes / s: the floor's bandwidth
MAPS = {"1.0": (54, 54, 54, 26, 26, 26, 26, 12), "1.1": (55, 55, 27, 27, 13, 13, 13, 13)}      # the side of each module's map at 224 x 224


def shape():
    print(f"# one Fire module (squeeze 1x1 -> expand 1x1 | expand 3x3), batch {batch}, fp16; us per call (hipGraph replay; median of {reps} "
          f"alternated rounds, min..max)")
    seen, wins_all = set(), []
    for version in ("1.0", "1.1"):
        net = models.SqueezeNet(version, num_classes=10)
        for k, (mod, hw) in enumerate(zip(net.modules_in_order(), MAPS[version]), 1):
            cs, c1, c3 = (c._conv for c in (mod._conv, mod._conv_path1, mod._conv_path2))
            cin, sq, e1, e3 = mod.in_channels, cs.out_channels, c1.out_channels, c3.out_channels
            key = (hw, hw, cin, sq, e1, e3)
            if key in seen:
                print(f"## {version} _conv{k}: {key} measured above")
                continue
            seen.add(key)
            g = torch.Generator().manual_seed(hw + cin)
            r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
            w = [(r(sq, cin, 1, 1) / cin ** 0.5).to(dev), (0.1 * r(sq)).to(dev), (r(e1, sq, 1, 1) / sq ** 0.5).to(dev), (0.1 * r(e1)).to(dev),
                 (r(e3, sq, 3, 3) / (9 * sq) ** 0.5).to(dev), (0.1 * r(e3)).to(dev)]
            p = E.FireParams(*w, torch.float16)
            nb = 16
            x = torch.relu(r(nb, hw, hw, cin)).half().to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
            y = torch.zeros((batch, hw, hw, p.cout), dtype=torch.float16, device=dev)
            assert E.fire_module_takes(x, p)
            yf = E.fire_module(x, p, fused=True, out=y).clone()
            yl = E.fire_module(x, p, fused=False, out=y)
            d = (yf.float() - yl.float()).abs().max().item()
            del yf
            calls = 10
            out = ab({"fused": (lambda: E.fire_module(x, p, fused=True, out=y), calls, 5),
                      "layered": (lambda: E.fire_module(x, p, fused=False, out=y), calls, 5)}, reps)
            nbytes = batch * hw * hw * (cin + p.cout) * 2
            nbytes -= nbytes % 32
            copy = copy_floor(nbytes, calls, reps)
            floor = nbytes / HBM * 1e6                                                  # us
            print(f"## {version} _conv{k}: ({batch}, {hw}, {hw}, {cin}) -> squeeze {sq} -> {e1} | {e3}")
            for name, (med, lo, hi) in out.items():
                print(f"{name:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  = {med / floor:.2f} x the byte floor", flush=True)
            print(f"byte floor: {nbytes / 1e6:.1f} MB (x read once, y written once) at 8 TB/s = {floor:.1f} us; a device-to-device copy "
                  f"moving as many bytes takes {copy[0]:.1f} us ({copy[1]:.1f}..{copy[2]:.1f})")
            wins = out["fused"][2] < out["layered"][1]
            if wins:
                wins_all.append(key)
            print(f"max|fused - layered| on the seeded maps: {d:.3e}; fused / layered = {out['fused'][0] / out['layered'][0]:.4f}: "
                  f"{'the fused arm is faster beyond the spread' if wins else 'NOT faster beyond the spread'}; the router sends it to the "
                  f"{'fused' if E._fire_module_routed(hw, hw, p) else 'layered'} arm", flush=True)
            del x, y
    print(f"# shapes the fused arm wins beyond the spread: {sorted(wins_all)}; engine.FIRE_MODULE_WINS holds {sorted(E.FIRE_MODULE_WINS)}")


def model():
    for version in ("1.0", "1.1"):
        m = models.SqueezeNet(version)
        m.load_dict(seeded.fill(seeded.shapes_of(m), 91))
        m = m.to(dev).set_eval()
        x = torch.from_numpy(seeded.image_batch(16, 0)).to(dev).repeat(batch // 16, 1, 1, 1).contiguous()
        graphs, routed = {}, E._fire_module_routed
        for arm in ("fused", "routed", "off"):          # fused: every module on the launch, whatever the measured table says
            E.set_option("fire_module", arm != "off")
            E._fire_module_routed = (lambda *a: True) if arm == "fused" else routed
            try:
                with torch.no_grad():
                    graphs[arm] = GraphedForward(m, x)
            finally:
                E._fire_module_routed = routed
                E.set_option("fire_module", True)
        t = {k: [] for k in graphs}
        for _ in range(reps):
            for k in graphs:
                t[k].append(timed(lambda: graphs[k](), 5))
        print(f"# SqueezeNet {version} batch {batch}, 224 x 224, fp16, hipGraph replay; median of {reps} alternated rounds of 5 forwards (min..max)")
        for k in graphs:
            v = sorted(t[k])
            med = v[len(v) // 2]
            print(f"fire_module {k:6s}: {med / 1e3:8.3f} ms ({v[0] / 1e3:.3f}..{v[-1] / 1e3:.3f})  {batch / med * 1e6:8.0f} img/s", flush=True)
        out = {k: (g.static_out if isinstance(g.static_out, torch.Tensor) else g.static_out[0]) for k, g in graphs.items()}
        print(f"max|logit difference| fused vs off: {(out['fused'].float() - out['off'].float()).abs().max().item():.3e}")
        del graphs, m, x


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "shape,model"
    if "shape" in what:
        shape()
    if "model" in what:
        model()
