"""Res2Net measurements on one MI355X (fp16).
  shape: the hierarchical 3x3 chain of a stride-1 block at every distinct chain shape of Res2Net-50 26w x 4s (and, with `wide`, of
         14w x 8s) at 224 x 224, on seeded maps and trained-like seeded parameters, two arms alternated:
            fused     tlxmi_res2_chain
            layered   what the launch replaces, the option-off arm of the same build: tlxmi_conv2d -> tlxmi_affine_act (the add) ->
                      tlxmi_conv2d ... -> tlxmi_copy_channels
         `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue.  Beside it the byte floor: one read
         of x and one write of y at 8 TB/s (the nominal HBM bandwidth; a device-to-device copy of the same bytes is timed next to it).  The
         fused arm wins a shape only if its slowest round is faster than the layered arm's fastest one.  The times are hipGraph replay times
         between two events, NOT the engine probe's per-launch records.  Only a shape the fused arm wins belongs in
         engine.RES2_CHAIN_WINS.
  model: Res2Net-50 26w x 4s img/s as a hipGraph replay (graph.GraphedForward), three arms alternated: every chain forced onto the launch,
         the default route (the measured table) and "res2chain" off.
usage: python tools/res2net_bench.py [batch=256] [reps=5] [shape,model[,wide]]"""
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


def chain_shapes(scales, width):
    """-> ordered {(hw, w, wp, scales): [block names]}: the distinct chains of a variant at 224 x 224."""
    net = models.Res2Net(scales=scales, width=width, class_num=10)
    hw, out = 56, {}
    for i, b in enumerate(net.block_list):
        if b.stride == 2:
            hw //= 2
        else:
            out.setdefault((hw, b.w, b.wp, b.scales), []).append(str(i))
    return out


def shape(variants):
    print(f"# one hierarchical 3x3 chain (conv, add, conv, add, ..., copy), batch {batch}, fp16; us per call (hipGraph replay; median of {reps} "
          f"alternated rounds, min..max)")
    for scales, width in variants:
        for (hw, w, wp, S), where in chain_shapes(scales, width).items():
            g = torch.Generator().manual_seed(hw + w + S)
            r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
            filters = [(r(w, w, 3, 3) * (2.0 / (9 * w)) ** 0.5).to(dev) for _ in range(S - 1)]
            bns = [((torch.rand(w, generator=g) * 0.4 + 0.8).to(dev), (r(w) * 0.05).to(dev)) for _ in range(S - 1)]
            params = E.Res2ChainParams(filters, bns, w, wp, torch.float16)
            nb = 16
            x = r(nb, hw, hw, S * wp).half()
            for s in range(S):
                x[..., s * wp + w:(s + 1) * wp] = 0
            x = torch.relu(x).to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
            y = torch.empty_like(x)
            assert E.res2_chain_takes(x, w, wp, S, E.ACT_RELU)
            rf = E.res2_chain(x, params, E.ACT_RELU, fused=True)
            rl = E.res2_chain(x, params, E.ACT_RELU, fused=False)
            d = (rf.float() - rl.float()).abs().max().item()
            del rf, rl
            calls = 10
            out = ab({"fused": (lambda: E.res2_chain(x, params, E.ACT_RELU, fused=True, out=y), calls, 5),
                      "layered": (lambda: E.res2_chain(x, params, E.ACT_RELU, fused=False, out=y), calls, 5)}, reps)
            nbytes = 2 * batch * hw * hw * S * w * 2
            nbytes -= nbytes % 32
            copy = copy_floor(2 * nbytes, calls, reps)      # (a copy OF nbytes: as many read and as many written)
            floor = nbytes / HBM * 1e6                                                  # us
            print(f"## {width}w x {scales}s blocks {' '.join(where)}: ({batch}, {hw}, {hw}, {S} x {w} at pitch {wp}), {S - 1} convs")
            for k, (med, lo, hi) in out.items():
                print(f"{k:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  = {med / floor:.2f} x the byte floor", flush=True)
            print(f"byte floor: {nbytes / 1e6:.1f} MB (the map read once, written once) at 8 TB/s = {floor:.1f} us; a device-to-device copy of the same "
                  f"bytes takes {copy[0]:.1f} us ({copy[1]:.1f}..{copy[2]:.1f})")
            wins = out["fused"][2] < out["layered"][1]
            print(f"max|fused - layered| on the seeded maps: {d:.3e}; fused / layered = {out['fused'][0] / out['layered'][0]:.4f}: "
                  f"{'the fused arm is faster beyond the spread' if wins else 'NOT faster beyond the spread'}; the router sends it to the "
                  f"{'fused' if E._res2_chain_routed(hw, hw, w, S) else 'layered'} arm", flush=True)
            del x, y


def model():
    m = models.res2net()
    m.load_dict(seeded.fill(seeded.shapes_of(m), 71))
    m = m.to(dev).set_eval()
    x = torch.from_numpy(seeded.image_batch(16, 0)).to(dev).repeat(batch // 16, 1, 1, 1).contiguous()
    graphs, routed = {}, E._res2_chain_routed
    for arm in ("fused", "routed", "off"):          # fused: every chain on the launch, whatever the measured table says
        E.set_option("res2chain", arm != "off")
        E._res2_chain_routed = (lambda *a: True) if arm == "fused" else routed
        try:
            with torch.no_grad():
                graphs[arm] = GraphedForward(m, x)
        finally:
            E._res2_chain_routed = routed
            E.set_option("res2chain", True)
    t = {k: [] for k in graphs}
    for _ in range(reps):
        for k in graphs:
            t[k].append(timed(lambda: graphs[k](), 5))
    print(f"# Res2Net-50 26w x 4s batch {batch}, 224 x 224, fp16, hipGraph replay; median of {reps} alternated rounds of 5 forwards (min..max)")
    for k in graphs:
        v = sorted(t[k])
        med = v[len(v) // 2]
        print(f"res2chain {k:6s}: {med / 1e3:8.3f} ms ({v[0] / 1e3:.3f}..{v[-1] / 1e3:.3f})  {batch / med * 1e6:8.0f} img/s", flush=True)
    d = (graphs["fused"].static_out.float() - graphs["off"].static_out.float()).abs().max().item()
    print(f"max|logit difference| fused vs off: {d:.3e}")


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "shape,model"
    if "shape" in what:
        shape([(4, 26)] + ([(8, 14)] if "wide" in what else []))
    if "model" in what:
        model()
