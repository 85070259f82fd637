"""ConvNeXt measurements on one MI355X (fp16).
  kernel: tlxmi_dwconv7_stats (conv + row statistics, one launch) against tlxmi_dwconv2d + tlxmi_layernorm (the "dwconv7"-off arm:
          conv, then the LayerNorm pass the fold removes) on the four stage shapes of ConvNeXt-T at 224 x 224, alternated; algorithmic
          bytes (input + output of the conv once, fp16) over time, against the measured copy rate of profiles/r01/roofline_denominators.txt.
  model:  ConvNeXt-T img/s as a hipGraph replay with "dwconv7" on and off, alternated.
usage: python tools/convnext_bench.py [batch=256] [reps=5]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, models  # noqa: E402
from tools.ab import model_on_off, timed  # noqa: E402

COPY_TBS = 4.75          # profiles/r01/roofline_denominators.txt: copy 1 GiB -> 1 GiB, read + write
dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def kernels():
    print(f"# kernel A/B, batch {batch}, fp16; us per call (hipGraph replay of 20 calls; median of {reps} alternated rounds of 10 replays, min..max); GB/s = conv input + output once")
    g = torch.Generator().manual_seed(0)
    for hw, c in ((56, 96), (28, 192), (14, 384), (7, 768)):
        x = torch.randn(batch, hw, hw, c, generator=g).half().to(dev)
        w = (torch.randn(7, 7, c, generator=g) / 7).half().to(dev)
        b = (0.1 * torch.randn(c, generator=g)).to(dev)
        gamma, beta = torch.ones(c, device=dev), torch.zeros(c, device=dev)

        def new():
            return E.dwconv7_stats(x, w, b, fused=True)

        def new_nostats():
            return E.dwconv7_stats(x, w, b, stats=False, fused=True)

        def old_conv():
            return E.dwconv7_stats(x, w, b, fused=False)

        def old():
            y, _ = E.dwconv7_stats(x, w, b, fused=False)
            return E.layernorm(y, gamma, beta, 1e-6)
        arms = (("dwconv7_stats", new), ("dwconv7 (no stats)", new_nostats), ("dwconv2d", old_conv), ("dwconv2d + layernorm", old))
        graphs = {}
        for k, f in arms:              # 20 calls of an arm as one hipGraph: the replay times kernels, not the host's enqueue
            for _ in range(10):
                f()
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                for _ in range(20):
                    f()
            graphs[k].replay()
        torch.cuda.synchronize()
        t = {k: [] for k, _ in arms}
        for _ in range(reps):
            for k, _ in arms:
                t[k].append(timed(graphs[k].replay, 10) / 20)
        nbytes = 2 * x.numel() * 2
        for k, _ in arms:
            v = sorted(t[k])
            med = v[len(v) // 2]
            print(f"{hw:3d}x{hw:<3d} C={c:4d}  {k:22s} {med:8.1f} us ({v[0]:.1f}..{v[-1]:.1f})  {nbytes / med / 1e3:7.0f} GB/s = {nbytes / med / 1e6 / COPY_TBS * 100:5.1f} % of the copy rate", flush=True)


def model():
    model_on_off("dwconv7", [("ConvNeXt-T", models.convnext, 1)], batch, reps, forwards=20, ms_width=7)


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "kernels,model"
    if "kernels" in what:
        kernels()
    if "model" in what:
        model()
