"""Twins (gvt) measurements on one MI355X (fp16).
  kernel: the attention half of a GSA block at the stage-1 and stage-2 shapes of alt_gvt_small and pcpvt_small (batch x 3136 tokens x 64
          channels, 2 heads / 1 head; batch x 784 x 128, 4 heads / 2 heads; 49 keys) on seeded rows and trained-like seeded parameters,
          the stream updated in place as the model runs it, three arms alternated:
            fused     tlxmi_gsa_block, the weight fragments staged in LDS (the product's choice)
            fused_l2  the same kernel reading the weight fragments from global memory (the tuning flavour's TLXMI_GSA_WLDS=0: a smaller
                      LDS footprint, more workgroups a CU)
            layers    what the fused launch replaces in the model, the option-off arm of the same build: q Linear on the normalised map
                      -> tlxmi_sr_attention -> proj Linear with the residual, written in place (norm1 itself runs in both arms of the model:
                      the keys are made of its output)
          `calls` calls of an arm as one hipGraph, so the replay times kernels and not the host's enqueue.  Beside it the byte floor:
          x read once, y written once, K / V and the parameter block read once, at the copy bandwidth measured here by a device-to-device
          copy of the same number of bytes (read + write counted).  The fused arm keeps a shape only if its slowest round is faster
          than the layers arm's fastest one.
          The times are hipGraph replay times between two events, NOT the engine probe's per-launch records.
  model:  alt_gvt_small and pcpvt_small img/s as a hipGraph replay (graph.GraphedForward) with "gsa_block" on and off, alternated.
usage: python tools/gvt_bench.py [batch=256] [reps=5] [kernel,model]"""
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

SHAPES = [("alt_gvt_small stage 1", 3136, 64, 2), ("alt_gvt_small stage 2", 784, 128, 4), ("pcpvt_small stage 1", 3136, 64, 1),
          ("pcpvt_small stage 2", 784, 128, 2)]


class _Layer:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def kernel():
    print(f"# the attention half of a GSA block, batch {batch}, 49 keys, fp16; us per call (hipGraph replay; median of {reps} alternated rounds, "
          "min..max)")
    for name, Lq, Cc, heads in SHAPES:
        g = torch.Generator().manual_seed(Lq + Cc + heads)
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        norm = _Layer(gamma=(torch.rand(Cc, generator=g) * 0.4 + 0.8).to(dev), beta=(r(Cc) * 0.05).to(dev))
        q = _Layer(weights=(r(Cc, Cc) * 1.5 / Cc ** 0.5).to(dev), biases=(r(Cc) * 0.02).to(dev))
        # proj at a tenth of the trained-like size: the stream is updated in place call after call and must stay far inside fp16
        proj = _Layer(weights=(r(Cc, Cc) * 0.1 / Cc ** 0.5).to(dev), biases=(r(Cc) * 0.002).to(dev))
        packed = E.gsa_block_params(norm, q, proj)
        x0 = (1.5 * r(16, Lq, Cc)).half().to(dev).repeat(batch // 16, 1, 1).contiguous()
        kv = r(16, 49, 2 * Cc).half().to(dev).repeat(batch // 16, 1, 1).contiguous()
        scale, eps = (Cc // heads) ** -0.5, 1e-6
        y_f = E.gsa_block(x0, packed, kv, heads, scale, eps, fused=True)
        y_l = E.gsa_block(x0, packed, kv, heads, scale, eps, fused=False)
        d = (y_f.float() - y_l.float()).abs().max().item()
        x = x0.clone()
        n = E.layernorm(x0, packed.gamma, packed.beta, eps)
        pkq, pkp = packed.linears(torch.float16)

        def layers():
            o = E.sr_attention(E.linear(n, pkq, packed.bq), kv, heads, scale)
            E.linear(o, pkp, packed.bp, res=x, out=x)

        fused = lambda: E.gsa_block(x, packed, kv, heads, scale, eps, fused=True, out=x)      # noqa: E731
        res = ab({"fused": (fused, 10, 5, None), "fused_l2": (fused, 10, 5, {"TLXMI_GSA_WLDS": "0"}), "layers": (layers, 10, 5, None)}, reps)
        assert torch.isfinite(x).all()
        nbytes = (2 * batch * Lq * Cc + batch * 49 * 2 * Cc) * 2 + packed.block.numel() * 2
        copy = copy_floor(nbytes, 10, reps)
        bw = nbytes / copy[0] / 1e3                                             # GB/s: nbytes / 2 read + nbytes / 2 written
        print(f"## {name}: ({batch}, {Lq}, 49, {Cc}, {heads} heads)")
        for k, (med, lo, hi) in res.items():
            print(f"{k:8s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  {nbytes / med / 1e3:7.1f} GB/s of x + y + K / V + parameters", flush=True)
        print(f"byte floor: {nbytes / 1e6:.1f} MB at the measured copy bandwidth of {bw:.0f} GB/s ({copy[0]:.1f} us for the same bytes, "
              f"{copy[1]:.1f}..{copy[2]:.1f}); fused / floor = {res['fused'][0] / copy[0]:.2f}")
        keeps = res["fused"][2] < res["layers"][1]
        print(f"max|fused - layers| on the seeded rows: {d:.3e}; fused / layers = {res['fused'][0] / res['layers'][0]:.4f}: "
              f"{'the fused arm is faster beyond the spread' if keeps else 'NOT faster beyond the spread: route this shape to the layers'}; "
              f"fused_l2 / fused = {res['fused_l2'][0] / res['fused'][0]:.4f}", flush=True)


def model():
    model_on_off("gsa_block", [(n, getattr(models, n), s) for n, s in (("alt_gvt_small", 17), ("pcpvt_small", 17))], batch, reps)


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "kernel,model"
    if "kernel" in what:
        kernel()
    if "model" in what:
        model()
