"""GoogLeNet measurements on one MI355X (fp16).
  shape: the head of each of the nine Inception modules (everything that reads the module's input) at 224 x 224 sizes, on seeded maps
         and seeded filters, two arms alternated:
            fused     tlxmi_inception_head
            layered   what the launch replaces, the option-off arm of the same build: tlxmi_conv2d x 3 -> tlxmi_maxpool2d -> tlxmi_conv2d
         `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue.  Beside it the byte floor: one
         read of x and one write of the four results at 8 TB/s (the nominal HBM bandwidth; a device-to-device copy of the same bytes is
         timed next to it).  The fused arm wins a shape only if its slowest round is faster than the layered arm's fastest one.  The times
         are hipGraph replay times between two events, NOT the engine probe's per-launch records.  Only a shape the fused arm wins
         belongs in engine.INCEPTION_HEAD_WINS.
  model: GoogLeNet img/s as a hipGraph replay (graph.GraphedForward), three arms alternated: every module forced onto the launch, the
         default route (the measured table) and "inception_head" off.
usage: python tools/googlenet_bench.py [batch=256] [reps=5] [shape,model]"""
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
MAPS = (27, 27, 13, 13, 13, 13, 13, 6, 6)      # the side of each module's map at 224 x 224


def shape():
    print(f"# the head of one Inception module (1x1 x 3, pool -> 1x1), batch {batch}, fp16; us per call (hipGraph replay; median of {reps} "
          f"alternated rounds, min..max)")
    net = models.GoogLeNet(num_classes=10)
    for mod, hw, name in zip(net.modules_in_order(), MAPS, ("3a", "3b", "4a", "4b", "4c", "4d", "4e", "5a", "5b")):
        cin = mod.in_channels
        g = torch.Generator().manual_seed(hw + cin)
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        ws = [(r(c._conv.out_channels, cin, 1, 1) / cin ** 0.5).to(dev) for c in (mod._conv1, mod._conv3r, mod._conv5r, mod._convprj)]
        p = E.InceptionParams(*ws, mod._conv3._conv.out_channels, mod._conv5._conv.out_channels, torch.float16)
        nb = 16
        x = torch.relu(r(nb, hw, hw, cin)).half().to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
        y = torch.zeros((batch, hw, hw, p.cout), dtype=torch.float16, device=dev)
        t = torch.zeros((batch, hw, hw, p.t_ld), dtype=torch.float16, device=dev)
        assert E.inception_head_takes(x, p)
        yf, tf = (v.clone() for v in E.inception_head(x, p, fused=True, out=y, mid=t))
        yl, tl = E.inception_head(x, p, fused=False, out=y, mid=t)
        d = max((yf.float() - yl.float()).abs().max().item(), (tf.float() - tl.float()).abs().max().item())
        del yf, tf
        calls = 10
        out = ab({"fused": (lambda: E.inception_head(x, p, fused=True, out=y, mid=t), calls, 5),
                  "layered": (lambda: E.inception_head(x, p, fused=False, out=y, mid=t), calls, 5)}, reps)
        nout = p.f1 + p.f3r + p.f5r + p.proj
        nbytes = batch * hw * hw * (cin + nout) * 2
        nbytes -= nbytes % 32
        copy = copy_floor(nbytes, calls, reps)
        floor = nbytes / HBM * 1e6                                                  # us
        print(f"## _ince{name}: ({batch}, {hw}, {hw}, {cin}) -> {p.f1} | {p.f3r} | {p.f5r} | {p.proj}")
        for k, (med, lo, hi) in out.items():
            print(f"{k:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  = {med / floor:.2f} x the byte floor", flush=True)
        print(f"byte floor: {nbytes / 1e6:.1f} MB (x read once, the four results written once) at 8 TB/s = {floor:.1f} us; a device-to-device copy "
              f"moving as many bytes takes {copy[0]:.1f} us ({copy[1]:.1f}..{copy[2]:.1f})")
        wins = out["fused"][2] < out["layered"][1]
        print(f"max|fused - layered| on the seeded maps: {d:.3e}; fused / layered = {out['fused'][0] / out['layered'][0]:.4f}: "
              f"{'the fused arm is faster beyond the spread' if wins else 'NOT faster beyond the spread'}; the router sends it to the "
              f"{'fused' if E._inception_head_routed(hw, hw, p) else 'layered'} arm", flush=True)
        del x, y, t


def model():
    m = models.googlenet()
    m.load_dict(seeded.fill(seeded.shapes_of(m), 86))
    m = m.to(dev).set_eval()
    x = torch.from_numpy(seeded.image_batch(16, 0)).to(dev).repeat(batch // 16, 1, 1, 1).contiguous()
    graphs, routed = {}, E._inception_head_routed
    for arm in ("fused", "routed", "off"):          # fused: every module on the launch, whatever the measured table says
        E.set_option("inception_head", arm != "off")
        E._inception_head_routed = (lambda *a: True) if arm == "fused" else routed
        try:
            with torch.no_grad():
                graphs[arm] = GraphedForward(m, x)
        finally:
            E._inception_head_routed = routed
            E.set_option("inception_head", True)
    t = {k: [] for k in graphs}
    for _ in range(reps):
        for k in graphs:
            t[k].append(timed(lambda: graphs[k](), 5))
    print(f"# GoogLeNet batch {batch}, 224 x 224, fp16, hipGraph replay; median of {reps} alternated rounds of 5 forwards (min..max)")
    for k in graphs:
        v = sorted(t[k])
        med = v[len(v) // 2]
        print(f"inception_head {k:6s}: {med / 1e3:8.3f} ms ({v[0] / 1e3:.3f}..{v[-1] / 1e3:.3f})  {batch / med * 1e6:8.0f} img/s", flush=True)
    d = max((a.float() - b.float()).abs().max().item() for a, b in zip(graphs["fused"].static_out, graphs["off"].static_out))
    print(f"max|logit difference| fused vs off, over the three heads: {d:.3e}")


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "shape,model"
    if "shape" in what:
        shape()
    if "model" in what:
        model()
