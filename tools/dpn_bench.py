"""DPN measurements on one MI355X (fp16).
  shape: each distinct `c` conv of DPN-68 and DPN-107 at 224 x 224 (one per stage: eight shapes), at the stage's last block (the widest
         dense_off), on seeded operands, two arms alternated:
            fused     tlxmi_dual_path_conv1x1
            layered   what the launch replaces, the option-off arm of the same build: tlxmi_conv2d on filter rows [0, bw) with
                      res = out = state, then on rows [bw, bw + inc) into the column slice
         `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue (the state accumulates from
         call to call: the addend is fixed, the sums stay far inside fp16 over the few hundred calls made).  Beside it the byte floor: t
         read once, the residual columns read and written once, the dense columns written once, at 8 TB/s (the nominal HBM bandwidth).
         The fused arm wins a shape only if its slowest round is faster than the layered arm's fastest one.  Only a shape the fused arm
         wins belongs in engine.DUAL_PATH_WINS.
  model: DPN-68 and DPN-107 img/s as a hipGraph replay (graph.GraphedForward), three arms alternated: every `c` conv forced onto the
         launch, the default route (the measured table) and "dual_path" off.
usage: python tools/dpn_bench.py [batch=256] [reps=5] [shape,model] [layers=68,107]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, seeded, models  # noqa: E402
from tlxcv_amd.graph import GraphedForward  # noqa: E402
from tlxcv_amd.models.classification.dpn import Layout  # noqa: E402
from tools.ab import ab, timed  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
what = sys.argv[3] if len(sys.argv) > 3 else "shape,model"
nets = [int(v) for v in (sys.argv[4] if len(sys.argv) > 4 else "68,107").split(",")]
HBM = 8.0e12        # bytes / s: the floor's bandwidth
SIDES = (56, 28, 14, 7)      # the side of each stage's map at 224 x 224


def shape():
    print(f"# one `c` conv (1x1: add onto [0, bw) in place | append inc at dense_off), batch {batch}, fp16; us per call (hipGraph replay; median "
          f"of {reps} alternated rounds, min..max)")
    seen, wins_all = set(), []
    for layers in nets:
        net = models.DPN(layers=layers, class_num=10)
        for (bw, inc, blocks), hw in zip(net.stages, SIDES):
            K = blocks[-1].c1x1_c_func.num_channels
            incp = (inc + 7) // 8 * 8
            off, ld = Layout.stage(bw, inc, len(blocks) - 1).width, Layout.stage(bw, inc, len(blocks)).width
            key = (hw * hw, K, bw, incp)
            if key in seen:
                print(f"## dpn{layers} {hw} x {hw}: {key} measured above")
                continue
            seen.add(key)
            g = torch.Generator().manual_seed(hw + K)
            r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
            p = E.DualPathParams((r(bw + incp, K, 1, 1) / K ** 0.5).to(dev), bw, torch.float16)
            nb = 16
            t = torch.relu(r(nb, hw, hw, K)).half().to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
            s0 = r(nb, hw, hw, ld).half().to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
            assert E.dual_path_takes(t, p, s0, off)
            sf, sl = s0.clone(), s0.clone()
            E.dual_path_conv1x1(t, p, sf, bw, off, fused=True)
            E.dual_path_conv1x1(t, p, sl, bw, off, fused=False)
            d = (sf.float() - sl.float()).abs().max().item()
            del sl
            sf.copy_(s0)
            calls = 10
            out = ab({"fused": (lambda: E.dual_path_conv1x1(t, p, sf, bw, off, fused=True), calls, 5),
                      "layered": (lambda: E.dual_path_conv1x1(t, p, sf, bw, off, fused=False), calls, 5)}, reps)
            rows = batch * hw * hw
            nbytes = rows * (K + 2 * bw + incp) * 2 + (bw + incp) * K * 2
            floor = nbytes / HBM * 1e6                                                  # us
            print(f"## dpn{layers} {hw} x {hw}: rows {rows}, K {K}, bw {bw}, inc {incp}, dense_off {off}, pitch {ld}")
            for name, (med, lo, hi) in out.items():
                print(f"{name:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  = {med / floor:.2f} x the byte floor", flush=True)
            print(f"byte floor: {nbytes / 1e6:.1f} MB (t read, the residual columns read and written, the dense columns written, the filter) at 8 TB/s = {floor:.1f} us")
            wins = out["fused"][2] < out["layered"][1]
            if wins:
                wins_all.append(key)
            print(f"max|fused - layered| on the seeded operands: {d:.3e}; fused / layered = {out['fused'][0] / out['layered'][0]:.4f}: "
                  f"{'the fused arm is faster in every round' if wins else 'NOT faster in every round'}; the router sends it to the "
                  f"{'fused' if E._dual_path_routed(hw * hw, p) else 'layered'} arm", flush=True)
            del t, s0, sf
    print(f"# shapes (pixels per image, K, bw, inc) the fused arm wins in every round: {sorted(wins_all)}; engine.DUAL_PATH_WINS holds {sorted(E.DUAL_PATH_WINS)}")


def model():
    for layers in nets:
        m = models.DPN(layers=layers)
        m.load_dict(seeded.fill(seeded.shapes_of(m), 101))
        m = m.to(dev).set_eval()
        x = torch.from_numpy(seeded.image_batch(16, 0)).to(dev).repeat(batch // 16, 1, 1, 1).contiguous()
        graphs, routed = {}, E._dual_path_routed
        for arm in ("fused", "routed", "off"):          # fused: every `c` conv on the launch, whatever the measured table says
            E.set_option("dual_path", arm != "off")
            E._dual_path_routed = (lambda *a: True) if arm == "fused" else routed
            try:
                with torch.no_grad():
                    graphs[arm] = GraphedForward(m, x)
            finally:
                E._dual_path_routed = routed
                E.set_option("dual_path", True)
        t = {k: [] for k in graphs}
        for _ in range(reps):
            for k in graphs:
                t[k].append(timed(lambda: graphs[k](), 3))
        print(f"# DPN-{layers} batch {batch}, 224 x 224, fp16, hipGraph replay; median of {reps} alternated rounds of 3 forwards (min..max)")
        for k in graphs:
            v = sorted(t[k])
            med = v[len(v) // 2]
            print(f"dual_path {k:6s}: {med / 1e3:8.3f} ms ({v[0] / 1e3:.3f}..{v[-1] / 1e3:.3f})  {batch / med * 1e6:8.0f} img/s", flush=True)
        out = {k: (g.static_out if isinstance(g.static_out, torch.Tensor) else g.static_out[0]) for k, g in graphs.items()}
        print(f"max|logit difference| fused vs off: {(out['fused'].float() - out['off'].float()).abs().max().item():.3e}")
        del graphs, m, x


if __name__ == "__main__":
    if "shape" in what:
        shape()
    if "model" in what:
        model()
