"""HarDNet measurements on one MI355X (fp16).
  shape: each distinct multi-link conv of HarDNet-85 (3x3) and HarDNet-39ds (1x1) at 224 x 224, on the block buffer of the model's own
         layout with seeded weights, two arms alternated:
            launch    tlxmi_link_conv2d: the linked slices read in place
            layered   what the launch replaces, the option-off arm of the same build: one tlxmi_copy_channels a link into a scratch
                      map, then tlxmi_conv2d on the same packed filter
         `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue.  Beside it the byte floor:
         the linked slices read once, the output written once, the filter, at 8 TB/s (the nominal HBM bandwidth).
         The launch wins a shape only if its slowest round is faster than the layered arm's fastest one.  Only a shape the launch
         wins belongs in engine.LINK_CONV_WINS.
  model: HarDNet-85 and HarDNet-39ds img/s as a hipGraph replay (graph.GraphedForward), three arms alternated: every multi-link conv
         forced onto the launch, the default route (the measured table; when the shape section ran in this process, the wins it just
         measured, and the line says so) and "link_conv" off.
usage: python tools/hardnet_bench.py [batch=256] [reps=5] [shape,model] [archs=85,39]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, seeded, models  # noqa: E402
from tlxcv_amd.graph import GraphedForward  # noqa: E402
from tools.ab import ab, timed  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
what = sys.argv[3] if len(sys.argv) > 3 else "shape,model"
nets = [int(v) for v in (sys.argv[4] if len(sys.argv) > 4 else "85,39").split(",")]
HBM = 8.0e12        # bytes / s: the floor's bandwidth
SIDES = {85: (56, 28, 28, 14, 14, 7), 39: (56, 28, 14, 7)}      # the side of each block's map at 224 x 224
measured = None     # the wins of the shape section of this process


def _net(arch):
    m = models.HarDNet(arch=arch, depth_wise=arch == 39, class_num=1000)
    m.load_dict(seeded.fill(seeded.shapes_of(m), 111))
    return m.to(dev).set_eval()


def shape():
    global measured
    print(f"# one multi-link conv (R x R over the concat of the linked slices of the block buffer), batch {batch}, fp16; us per call (hipGraph replay; "
          f"median of {reps} alternated rounds, min..max)")
    seen, wins_all = set(), []
    for arch in nets:
        net = _net(arch)
        for bi, (blk, hw) in enumerate(zip(net.blocks(), SIDES[arch])):
            lay = blk.layout
            g = torch.Generator().manual_seed(hw + lay.ld)
            nb = 16
            buf = torch.rand(nb, hw, hw, lay.ld, generator=g).mul_(6).half().to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
            rows = batch * hw * hw
            for L, (m, (conv, link, widths)) in enumerate(zip(blk.layers, blk.link_convs()), start=1):
                if len(link) < 2:
                    continue
                segs, p = lay.segments(link), conv.link_params(widths)
                key = (hw * hw, p.R, tuple(c for _, c in segs), p.Cout)
                tag = f"hardnet{arch}{'ds' if arch == 39 else ''} block {bi + 1} layer {L} {hw} x {hw}"
                if key in seen:
                    print(f"## {tag}: {key} measured above")
                    continue
                seen.add(key)
                inplace = p.R == 3          # the 1x1 of a depth_wise layer writes a temporary, the 3x3 its slice of the buffer
                out = buf[..., lay.off[L]:lay.off[L] + lay.width[L]] if inplace else torch.empty((batch, hw, hw, p.Cout), dtype=buf.dtype, device=dev)
                out_ld = lay.ld if inplace else p.Cout
                assert E.link_conv_takes(buf, segs, p, E.ACT_RELU6, out, out_ld)
                E.link_conv2d(buf, segs, p, E.ACT_RELU6, out, out_ld, fused=True)
                a = out.clone()
                E.link_conv2d(buf, segs, p, E.ACT_RELU6, out, out_ld, fused=False)
                d = (a.float() - out.float()).abs().max().item()
                del a
                calls = 5
                res = ab({"launch": (lambda: E.link_conv2d(buf, segs, p, E.ACT_RELU6, out, out_ld, fused=True), calls, 3),
                          "layered": (lambda: E.link_conv2d(buf, segs, p, E.ACT_RELU6, out, out_ld, fused=False), calls, 3)}, reps)
                nbytes = rows * (p.K + p.Cout) * 2 + p.Cout * p.K * p.R * p.R * 2
                floor = nbytes / HBM * 1e6                                                  # us
                print(f"## {tag}: rows {rows}, R {p.R}, links {link} = segments {segs}, K {p.K}, Cout {p.Cout}, pitch {lay.ld}")
                for name, (med, lo, hi) in res.items():
                    print(f"{name:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  = {med / floor:.2f} x the byte floor", flush=True)
                wins = res["launch"][2] < res["layered"][1]
                if wins:
                    wins_all.append(key)
                print(f"byte floor {floor:.1f} us ({nbytes / 1e6:.1f} MB); max|launch - layered| {d:.3e}; launch / layered = {res['launch'][0] / res['layered'][0]:.4f}: "
                      f"{'the launch is faster in every round' if wins else 'NOT faster in every round'}; the router sends it to the "
                      f"{'launch' if E._link_conv_routed(hw * hw, segs, p) else 'layers'}", flush=True)
                del out
            del buf
        del net
    measured = frozenset(wins_all)
    print(f"# shapes (pixels per image, R, link widths, Cout) the launch wins in every round: {sorted(wins_all)}")
    print(f"# engine.LINK_CONV_WINS holds {sorted(E.LINK_CONV_WINS)}")


def model():
    table = E.LINK_CONV_WINS
    if measured is not None and measured != table:
        print("# the default route below uses the wins measured ABOVE IN THIS RUN, not the committed table")
        E.LINK_CONV_WINS = measured
    try:
        for arch in nets:
            m = _net(arch)
            x = torch.from_numpy(seeded.image_batch(16, 0)).to(dev).repeat(batch // 16, 1, 1, 1).contiguous()
            graphs, routed = {}, E._link_conv_routed
            for arm in ("forced", "routed", "off"):          # forced: every multi-link conv on the launch, whatever the table says
                E.set_option("link_conv", arm != "off")
                E._link_conv_routed = (lambda *a: True) if arm == "forced" else routed
                try:
                    with torch.no_grad():
                        graphs[arm] = GraphedForward(m, x)
                finally:
                    E._link_conv_routed = routed
                    E.set_option("link_conv", True)
            t = {k: [] for k in graphs}
            for _ in range(reps):
                for k in graphs:
                    t[k].append(timed(lambda: graphs[k](), 3))
            print(f"# HarDNet-{arch}{'ds' if arch == 39 else ''} batch {batch}, 224 x 224, fp16, hipGraph replay; median of {reps} alternated rounds of 3 forwards (min..max)")
            for k in graphs:
                v = sorted(t[k])
                med = v[len(v) // 2]
                print(f"link_conv {k:6s}: {med / 1e3:8.3f} ms ({v[0] / 1e3:.3f}..{v[-1] / 1e3:.3f})  {batch / med * 1e6:8.0f} img/s", flush=True)
            out = {k: (g.static_out if isinstance(g.static_out, torch.Tensor) else g.static_out[0]) for k, g in graphs.items()}
            print(f"max|logit difference| forced vs off: {(out['forced'].float() - out['off'].float()).abs().max().item():.3e}")
            del graphs, m, x
    finally:
        E.LINK_CONV_WINS = table


if __name__ == "__main__":
    if "shape" in what:
        shape()
    if "model" in what:
        model()
