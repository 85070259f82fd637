"""CSWin-tiny measurements on one MI355X (fp16).
  stages: the attention of each of the four stages at 224 x 224 — engine.cswin_attention on a seeded packed qkv (B, H*W, 3C) with the
          stage's stripes and seeded LePE operands — with the MFMA arm (tlxmi_cswin_attention) and the plain arm
          (tlxmi_cswin_attention_plain) forced, alternated: `calls` calls of an arm as one hipGraph (10 for the MFMA arm, 2 for the plain
          one, which is not tuned and takes milliseconds), so the replay times kernels and not the host's enqueue.  The forward runs the
          stages at the batch it is given and, above the two-stream threshold, at half of it on two streams: both batches are timed.  The
          MFMA arm is also given in GB/s of its algorithmic bytes (q, k, v read once, out written once).  A stage keeps the MFMA arm only
          if its slowest round is faster than the plain arm's fastest one (the run-to-run spread printed beside each median).
          The times are hipGraph replay times between two events, NOT the engine probe's per-launch records: the probe brackets one
          eager launch with events and so includes the host's enqueue gap, which at 30 - 200 us a call is not negligible; the probe's
          bytes / flops formulas (engine.cswin_attention) are what the GB/s column uses.
  model:  CSWin-tiny img/s as a hipGraph replay with "cswin_attn" on and off, alternated.
usage: python tools/cswin_bench.py [batch=256] [reps=5] [stages,model]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, models  # noqa: E402
from tools.ab import ab, model_on_off  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
STAGES = ((1, 56, 2, 1), (2, 28, 4, 2), (3, 14, 8, 7), (4, 7, 16, None))      # (stage, H = W, heads, split; None = one branch, the whole map)


def stages():
    print(f"# per stage, CSWin-tiny at 224 x 224, fp16, head dim 32; us per call (hipGraph replay; median of {reps} alternated rounds, min..max)")
    g = torch.Generator().manual_seed(0)
    for b in (batch, batch // 2):
        for stage, hw, heads, split in STAGES:
            Cc = heads * 32
            splits = [(hw, hw)] if split is None else split
            qkv = torch.randn(b, hw * hw, 3 * Cc, generator=g).half().to(dev)
            w = (torch.randn(3, 3, Cc, generator=g) / 3).half().to(dev)
            bias = (torch.randn(Cc, generator=g) * 0.1).to(dev)
            run = lambda fused: E.cswin_attention(qkv, b, hw, hw, heads, splits, w, bias, 32 ** -0.5, fused=fused)      # noqa: E731
            arms = {"mfma": (lambda: run(True), 10, 5), "plain": (lambda: run(False), 2, 2)}
            outs = {k: f() for k, (f, _, _) in arms.items()}
            res = ab(arms, reps)
            tokens = E.cswin_stripes(hw, hw, splits)[0][0] * E.cswin_stripes(hw, hw, splits)[0][1]
            nbytes = 4 * b * hw * hw * Cc * 2
            for k, (med, lo, hi) in res.items():
                extra = f"  {nbytes / med / 1e3:7.1f} GB/s" if k == "mfma" else ""
                print(f"stage {stage} batch {b:4d} {hw}x{hw} heads {heads:2d} stripe {tokens:3d} tokens {k:5s} {med:10.1f} us ({lo:.1f}..{hi:.1f}){extra}",
                      flush=True)
            d = (outs["mfma"].float() - outs["plain"].float()).abs().max().item()
            keeps = res["mfma"][2] < res["plain"][1]
            print(f"stage {stage} batch {b:4d} max|mfma - plain| = {d:.3e}, mfma / plain = {res['mfma'][0] / res['plain'][0]:.4f}: "
                  f"{'the MFMA arm is faster beyond the spread' if keeps else 'NOT faster beyond the spread: route this stage to the plain arm'}", flush=True)
            del qkv
            torch.cuda.empty_cache()


def model():
    model_on_off("cswin_attn", [("CSWin-tiny", models.CSwintransformer_thiny, 16)], batch, reps, forwards=(10, 2))


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "stages,model"
    if "stages" in what:
        stages()
    if "model" in what:
        model()
