"""PVTv2-B0 measurements on one MI355X (fp16).
  stages: the attention of each of the four stages at 224 x 224 — engine.sr_attention on seeded q (B, Lq, C) and packed kv (B, 49, 2C) —
          with "sr_attn" on (tlxmi_sr_attention) and off (tlxmi_mha), alternated: 10 calls of an arm as one hipGraph, so the replay times
          kernels and not the host's enqueue.  The forward runs the stages at the batch it is given and, above the two-stream threshold,
          at half of it on two streams: both batches are timed.  Algorithmic bytes = q + out + kv once, fp16.
  model:  PVTv2-B0 img/s as a hipGraph replay with "sr_attn" on and off, alternated.
usage: python tools/pvt_v2_bench.py [batch=256] [reps=5] [stages,model]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, models  # noqa: E402
from tools.ab import model_on_off, timed  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
STAGES = ((1, 3136, 49, 1, 32), (2, 784, 49, 2, 32), (3, 196, 49, 5, 32), (4, 49, 49, 8, 32))      # (stage, Lq, Lk, heads, hd) at 224 x 224


def stages():
    print(f"# attention per stage, PVTv2-B0 at 224 x 224, fp16; us per call (hipGraph replay of 10 calls; median of {reps} alternated rounds of 5 "
          "replays, min..max); GB/s = q + out + kv once")
    g = torch.Generator().manual_seed(0)
    for b in (batch, batch // 2):
        for stage, Lq, Lk, heads, hd in STAGES:
            Cc = heads * hd
            q = torch.randn(b, Lq, Cc, generator=g).half().to(dev)
            kv = torch.randn(b, Lk, 2 * Cc, generator=g).half().to(dev)
            arms = (("sr_attention", True), ("mha", False))
            graphs, outs = {}, {}
            for k, fused in arms:
                def f(fused=fused):
                    return E.sr_attention(q, kv, heads, hd ** -0.5, fused=fused)
                for _ in range(3):
                    outs[k] = f()
                torch.cuda.synchronize()
                graphs[k] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[k]):
                    for _ in range(10):
                        f()
                graphs[k].replay()
            torch.cuda.synchronize()
            t = {k: [] for k, _ in arms}
            for _ in range(reps):
                for k, _ in arms:
                    t[k].append(timed(graphs[k].replay, 5) / 10)
            nbytes = (2 * b * Lq * Cc + b * Lk * 2 * Cc) * 2
            diff = (outs["sr_attention"].float() - outs["mha"].float()).abs().max().item()
            for k, _ in arms:
                v = sorted(t[k])
                med = v[len(v) // 2]
                print(f"stage {stage} batch {b:4d} Lq={Lq:4d} Lk={Lk} heads={heads} hd={hd}  {k:12s} {med:9.1f} us ({v[0]:.1f}..{v[-1]:.1f})  "
                      f"{nbytes / med / 1e3:7.0f} GB/s", flush=True)
            print(f"stage {stage} batch {b:4d} max|sr_attention - mha| = {diff:.3e}", flush=True)
            del q, kv, graphs, outs
            torch.cuda.empty_cache()


def model():
    model_on_off("sr_attn", [("PVTv2-B0", models.pvt_v2, 15)], batch, reps, forwards=10, ms_width=7)


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "stages,model"
    if "stages" in what:
        stages()
    if "model" in what:
        model()
