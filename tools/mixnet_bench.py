"""MixNet measurements on one MI355X (fp16).
  shape: one MixConv + BatchNorm + activation (+ the SE pool where the unit has an SE block) at every distinct shape of mixnet_s and
         mixnet_m at 224 x 224, on seeded maps and trained-like seeded parameters, two arms alternated:
            fused     tlxmi_mixconv_dw
            groups    what the launch replaces, the option-off arm of the same build: one tlxmi_dwconv2d a group (through dense copies where
                      a group does not start and end on 16-byte chunks) -> tlxmi_global_avgpool
         `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue.  Beside it the byte floor: one read
         of x and one write of y at 8 TB/s (the nominal HBM bandwidth; a device-to-device copy of the same bytes is timed next to it).  The
         fused arm wins a shape only if its slowest round is faster than the groups arm's fastest one.  The times are hipGraph replay times
         between two events, NOT the engine probe's per-launch records.
  model: mixnet_s, mixnet_m and mixnet_l img/s as a hipGraph replay (graph.GraphedForward) with "mixconv" on and off, alternated.
usage: python tools/mixnet_bench.py [batch=256] [reps=5] [shape,model]"""
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
HBM = 8.0e12        # bytes / s: the floor's bandwidth


def unit_shapes(name):
    """-> ordered {(hw, C, groups, stride, act, pool): "units"}: the distinct mixed depthwise convs of a variant at 224 x 224."""
    net = getattr(models, name)()
    hw, out = 112, {}
    for i, u in enumerate(net.units()):
        if u.mixed:
            key = (hw, u.mid_channels, len(u.conv1.conv.splitted_in_channels), u.stride, u.conv1._act, u.use_se)
            out.setdefault(key, []).append(str(i))
        if u.stride == 2:
            hw //= 2
    return out


def shape():
    print(f"# one MixConv + BN + act (+ SE pool), batch {batch}, fp16; us per call (hipGraph replay; median of {reps} alternated rounds, min..max)")
    seen = {}
    for name in ("mixnet_s", "mixnet_m"):
        for key, us in unit_shapes(name).items():
            seen.setdefault(key, []).append(f"{name[7:]}:{','.join(us)}")
    for (hw, Cc, G, st, act, pool), where in seen.items():
        g = torch.Generator().manual_seed(hw + Cc + G)
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        groups = models.MixConv.split_channels(Cc, G)
        kernels = [3 + 2 * i for i in range(G)]
        filters = [(r(n, 1, k, k) * (2.0 / (k * k)) ** 0.5).to(dev) for n, k in zip(groups, kernels)]
        params = E.MixConvParams(filters, ((torch.rand(Cc, generator=g) * 0.4 + 0.8).to(dev), (r(Cc) * 0.05).to(dev)), torch.float16)
        nb = 16 if hw <= 56 else 4
        x = r(nb, hw, hw, Cc).half().to(dev).repeat(batch // nb, 1, 1, 1).contiguous()
        ho = (hw - 1) // st + 1
        y = torch.empty((batch, ho, ho, Cc), dtype=torch.float16, device=dev)
        assert E.mixconv_dw_supported(x, groups, kernels, st, act, pool)
        rf = E.mixconv_dw(x, params, st, act, pool=pool, fused=True)
        rl = E.mixconv_dw(x, params, st, act, pool=pool, fused=False)
        d = ((rf[0] if pool else rf).float() - (rl[0] if pool else rl).float()).abs().max().item()
        dp = (rf[1].float() - rl[1].float()).abs().max().item() if pool else 0.0
        del rf, rl
        calls = 10 if hw <= 56 else 4
        out = ab({"fused": (lambda: E.mixconv_dw(x, params, st, act, pool=pool, fused=True, out=y), calls, 5),
                  "groups": (lambda: E.mixconv_dw(x, params, st, act, pool=pool, fused=False, out=y), calls, 5)}, reps)
        nbytes = (x.numel() + y.numel()) * 2
        nbytes -= nbytes % 32
        copy = copy_floor(nbytes, calls, reps)
        floor = nbytes / HBM * 1e6                                                  # us
        print(f"## units {' '.join(where)}: ({batch}, {hw}, {hw}, {Cc}) in {G} groups of {groups[0]}, windows {kernels}, stride {st}, "
              f"act {act}{', + SE pool' if pool else ''}")
        for k, (med, lo, hi) in out.items():
            print(f"{k:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  {nbytes / med / 1e3:7.1f} GB/s of the floor's bytes  = {med / floor:.2f} x the byte floor", flush=True)
        print(f"byte floor: {nbytes / 1e6:.1f} MB (x read once, y written once) at 8 TB/s = {floor:.1f} us; a device-to-device copy of the same bytes "
              f"takes {copy[0]:.1f} us ({copy[1]:.1f}..{copy[2]:.1f})")
        wins = out["fused"][2] < out["groups"][1]
        print(f"max|fused - groups| on the seeded maps: {d:.3e} (pool {dp:.3e}); fused / groups = {out['fused'][0] / out['groups'][0]:.4f}: "
              f"{'the fused arm is faster beyond the spread' if wins else 'NOT faster beyond the spread'}", flush=True)
        del x, y


def model():
    model_on_off("mixconv", [(n, getattr(models, n), s) for n, s in (("mixnet_s", 53), ("mixnet_m", 52), ("mixnet_l", 53))], batch, reps)


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "shape,model"
    if "shape" in what:
        shape()
    if "model" in what:
        model()
