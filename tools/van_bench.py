"""VAN-B0 measurements on one MI355X (fp16).
  stages: per stage shape at 224 x 224 — the depthwise chain (engine.lka_dw), the gated projection (engine.lka_gate), the whole attention
          half of a block (proj_1 + GELU, lka_dw, lka_gate: Attention.run_block) and the Mlp half (fc1, depthwise 3x3 + GELU, fc2 with the
          residual) — with the "lka" arms on (tlxmi_lka_dw / tlxmi_lka_gate forced for the two kernels; the engine's default dispatch, which
          keeps a fused kernel only where it measured faster, for the attention half) and off (tlxmi_dwconv2d x 2; tlxmi_conv2d, tlxmi_mul,
          tlxmi_affine_act, tlxmi_conv2d), alternated: 10 calls of an arm as one hipGraph, so the replay times kernels and not the host's
          enqueue.  The forward runs the stages at the batch it is given and, above the two-stream threshold, at half of it on two streams:
          both batches are timed.  lka_dw is also given as a share of `copy_tbs` (the copy rate of profiles/r01/roofline_denominators.txt)
          for its 2 passes over the N*H*W*C map.
  model:  VAN-B0 img/s as a hipGraph replay with "lka" on and off, alternated.
usage: python tools/van_bench.py [batch=256] [reps=5] [stages,model] [copy_tbs=4.75]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, seeded, models  # noqa: E402
from tools.ab import ab, model_on_off  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
copy_tbs = float(sys.argv[4]) if len(sys.argv) > 4 else 4.75
STAGES = ((1, 56, 32), (2, 28, 64), (3, 14, 160), (4, 7, 256))      # (stage, H = W, C) at 224 x 224


def stages():
    print(f"# per stage, VAN-B0 at 224 x 224, fp16; us per call (hipGraph replay of 10 calls; median of {reps} alternated rounds of 5 replays, "
          f"min..max); on = tlxmi_lka_dw / tlxmi_lka_gate, off = the pre-existing kernels only; copy rate {copy_tbs} TB/s")
    m = models.van()
    m.load_dict(seeded.fill(seeded.shapes_of(m), 16))
    m = m.to(dev).set_eval()
    g = torch.Generator().manual_seed(0)
    for b in (batch, batch // 2):
        for stage, hw, Cc in STAGES:
            blk = getattr(m, f"block{stage}")[0]
            att, lka = blk.attn, blk.attn.spatial_gating_unit
            x = torch.randn(b, hw, hw, Cc, generator=g).half().to(dev)
            with torch.no_grad():
                blk.run_nhwc(x)                                   # derived tensors
                t = torch.randn(b, hw, hw, Cc, generator=g).half().to(dev)
                w0, b0 = lka.conv0.packed(), lka.conv0.bias32()
                w1, b1 = lka.conv_spatial.packed(), lka.conv_spatial.bias32()
                a1 = E.lka_dw(t, w0, b0, w1, b1)
                pk1, c1, pk2, s2, h2, rs = att.gate_operands(blk.norm1, blk.layer_scale_1, blk)

                def half(on, which):
                    def f():
                        E.set_option("lka", on)
                        try:
                            return blk.run_attn(x) if which == "attn" else blk.run_mlp(x)
                        finally:
                            E.set_option("lka", True)
                    return f
                groups = (
                    ("lka_dw", {"on": lambda: E.lka_dw(t, w0, b0, w1, b1, fused=True), "off": lambda: E.lka_dw(t, w0, b0, w1, b1, fused=False)}),
                    ("lka_gate", {"on": lambda: E.lka_gate(a1, t, pk1, None, c1, pk2, s2, h2, x, rs, fused=True),
                                  "off": lambda: E.lka_gate(a1, t, pk1, None, c1, pk2, s2, h2, x, rs, fused=False)}),
                    ("attention half", {"on": half(True, "attn"), "off": half(False, "attn")}),
                    ("mlp half", {"only": half(True, "mlp")}),
                )
                for name, arms in groups:
                    outs = {k: f() for k, f in arms.items()}
                    res = ab({k: (f, 10, 5) for k, f in arms.items()}, reps)
                    for k, (med, lo, hi) in res.items():
                        extra = ""
                        if name == "lka_dw":
                            ideal = 2 * x.numel() * 2 / (copy_tbs * 1e12) * 1e6
                            extra = f"  {ideal / med * 100:5.1f} % of the copy rate for 2 passes ({ideal:.1f} us)"
                        print(f"stage {stage} batch {b:4d} {hw}x{hw}x{Cc:<3d} {name:15s} {k:4s} {med:9.1f} us ({lo:.1f}..{hi:.1f}){extra}", flush=True)
                    if len(outs) == 2:
                        d = (outs["on"].float() - outs["off"].float()).abs().max().item()
                        print(f"stage {stage} batch {b:4d} {name}: max|on - off| = {d:.3e}, on / off = {res['on'][0] / res['off'][0]:.2f}", flush=True)
            del x, t, a1
            torch.cuda.empty_cache()


def model():
    model_on_off("lka", [("VAN-B0", models.van, 16)], batch, reps, forwards=10, ms_width=7)


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "stages,model"
    if "stages" in what:
        stages()
    if "model" in what:
        model()
