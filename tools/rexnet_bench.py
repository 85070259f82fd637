"""ReXNet measurements on one MI355X (fp16).
  shape: each distinct projection of ReXNet-1.0 and ReXNet-2.0 at 224 x 224 — (pixels per image, K, Cout, res_c, gated), K and Cout at
         the padded pitch — on maps of the model's own layout with seeded weights, two arms alternated:
            launch    tlxmi_gated_conv1x1: gate, ReLU6, 1x1 conv + BN and the partial shortcut in one launch
            layered   what the launch replaces, the option-off arm of the same build: tlxmi_scale_channels -> tlxmi_affine_act ->
                      tlxmi_conv2d with the shortcut as its residual (through a zero-filled copy of its first res_c columns)
         `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue.  Beside it the byte floor:
         the operand read once, the shortcut read once, the output written once, the filter, at 8 TB/s (the nominal HBM bandwidth).
         The launch wins a shape only if its slowest round is faster than the layered arm's fastest one.  Only a shape the launch
         wins belongs in engine.GATED_CONV_WINS.
  model: ReXNet-1.0 and ReXNet-2.0 img/s as a hipGraph replay (graph.GraphedForward), three arms alternated: every projection forced
         onto the launch, the default route (the measured table; when the shape section ran in this process, the wins it just
         measured, and the line says so) and "gated_conv" off.
usage: python tools/rexnet_bench.py [batch=256] [reps=5] [shape,model] [archs=rexnet_1_0,rexnet_2_0]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, seeded, models  # noqa: E402
from tlxcv_amd.graph import GraphedForward  # noqa: E402
from tlxcv_amd.models.classification.rexnet import _padded_1x1, _up  # noqa: E402
from tools.ab import ab, timed  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
what = sys.argv[3] if len(sys.argv) > 3 else "shape,model"
nets = (sys.argv[4] if len(sys.argv) > 4 else "rexnet_1_0,rexnet_2_0").split(",")
HBM = 8.0e12        # bytes / s: the floor's bandwidth
measured = None     # the wins of the shape section of this process


def _net(arch):
    m = getattr(models, arch)(class_num=1000)
    m.load_dict(seeded.fill(seeded.shapes_of(m), 121))
    return m.to(dev).set_eval()


def shape():
    global measured
    print(f"# one projection (gate -> ReLU6 -> 1x1 conv + BN -> shortcut onto the first res_c channels), batch {batch}, fp16; us per call "
          f"(hipGraph replay; median of {reps} alternated rounds, min..max)")
    seen, wins_all = set(), []
    for arch in nets:
        net = _net(arch)
        side = 112
        for bi, b in enumerate(net.blocks()):
            side = (side - 1) // b.stride + 1
            proj, pbn = b.parts()[3]
            pk, s, t = _padded_1x1(proj, pbn)
            K, Cout, res_c = pk.Cin, pk.Cout, b.in_channels if b.use_shortcut else 0
            key = (side * side, K, Cout, res_c, b.use_se)
            tag = f"{arch} block {bi} {side} x {side}"
            if key in seen:
                print(f"## {tag}: {key} measured above")
                continue
            seen.add(key)
            g = torch.Generator().manual_seed(side + K)
            nb = 16
            x = torch.randn(nb, side, side, K, generator=g).mul_(4).half()
            x[..., b.dw_channels:] = 0
            x = x.to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
            gate = torch.rand(batch, K, generator=g).half().to(dev) if b.use_se else None
            res = None
            if res_c:
                res = torch.randn(nb, side, side, _up(res_c), generator=g).half()
                res[..., res_c:] = 0
                res = res.to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
            out = torch.empty((batch, side, side, Cout), dtype=torch.float16, device=dev)
            rows = batch * side * side
            assert E.gated_conv1x1_takes(x, gate, pk, res, res_c)
            run = lambda fused: E.gated_conv1x1(x, gate, pk, s, t, res=res, res_c=res_c, out=out, fused=fused)      # noqa: E731
            a = run(True).clone()
            d = (a.float() - run(False).float()).abs().max().item()
            del a
            calls = 5
            r = ab({"launch": (lambda: run(True), calls, 3), "layered": (lambda: run(False), calls, 3)}, reps)
            nbytes = rows * (K + Cout + _up(res_c)) * 2 + Cout * K * 2
            floor = nbytes / HBM * 1e6                                                  # us
            print(f"## {tag}: rows {rows}, K {K}, Cout {Cout}, res_c {res_c}, gated {b.use_se}")
            for name, (med, lo, hi) in r.items():
                print(f"{name:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  = {med / floor:.2f} x the byte floor", flush=True)
            wins = r["launch"][2] < r["layered"][1]
            if wins:
                wins_all.append(key)
            print(f"byte floor {floor:.1f} us ({nbytes / 1e6:.1f} MB); max|launch - layered| {d:.3e}; launch / layered = {r['launch'][0] / r['layered'][0]:.4f}: "
                  f"{'the launch is faster in every round' if wins else 'NOT faster in every round'}; the router sends it to the "
                  f"{'launch' if E._gated_conv_routed(side * side, pk, res_c, b.use_se) else 'layers'}", flush=True)
            del x, gate, res, out
        del net
    measured = frozenset(wins_all)
    print(f"# shapes (pixels per image, K, Cout, res_c, gated) the launch wins in every round: {sorted(wins_all)}")
    print(f"# engine.GATED_CONV_WINS holds {sorted(E.GATED_CONV_WINS)}")


def model():
    table = E.GATED_CONV_WINS
    if measured is not None and measured != table:
        print("# the default route below uses the wins measured ABOVE IN THIS RUN, not the committed table")
        E.GATED_CONV_WINS = measured
    try:
        for arch in nets:
            m = _net(arch)
            x = torch.from_numpy(seeded.image_batch(16, 0)).to(dev).repeat(batch // 16, 1, 1, 1).contiguous()
            graphs, routed = {}, E._gated_conv_routed
            for arm in ("forced", "routed", "off"):          # forced: every projection on the launch, whatever the table says
                E.set_option("gated_conv", arm != "off")
                E._gated_conv_routed = (lambda *a: True) if arm == "forced" else routed
                try:
                    with torch.no_grad():
                        graphs[arm] = GraphedForward(m, x)
                finally:
                    E._gated_conv_routed = routed
                    E.set_option("gated_conv", True)
            t = {k: [] for k in graphs}
            for _ in range(reps):
                for k in graphs:
                    t[k].append(timed(lambda: graphs[k](), 3))
            print(f"# {arch} batch {batch}, 224 x 224, fp16, hipGraph replay; median of {reps} alternated rounds of 3 forwards (min..max)")
            for k in graphs:
                v = sorted(t[k])
                med = v[len(v) // 2]
                print(f"gated_conv {k:6s}: {med / 1e3:8.3f} ms ({v[0] / 1e3:.3f}..{v[-1] / 1e3:.3f})  {batch / med * 1e6:8.0f} img/s", flush=True)
            out = {k: (g.static_out if isinstance(g.static_out, torch.Tensor) else g.static_out[0]) for k, g in graphs.items()}
            print(f"max|logit difference| forced vs off: {(out['forced'].float() - out['off'].float()).abs().max().item():.3e}")
            del graphs, m, x
    finally:
        E.GATED_CONV_WINS = table


if __name__ == "__main__":
    if "shape" in what:
        shape()
    if "model" in what:
        model()
