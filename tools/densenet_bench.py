"""DenseNet measurements on one MI355X (fp16).
  kernel: tlxmi_preact_conv1x1 (BatchNorm + ReLU on the A operand inside the 1x1-conv GEMM, one launch) against the "preact"-off pair
          (tlxmi_affine_act into a dense K-channel temporary, then tlxmi_conv2d) at DenseNet-121's shapes at 224 x 224: the first / middle /
          last dense layer of each block (a channel prefix of the block's buffer) and the three transitions, alternated; algorithmic bytes
          (the K input channels once + the output + the filter, fp16) over time, against the measured copy rate of
          profiles/r01/roofline_denominators.txt.
  model:  DenseNet-121 img/s as a hipGraph replay with "preact" on and off, alternated.
usage: python tools/densenet_bench.py [batch=256] [reps=5] [kernels,model]"""
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


def shapes():
    """(label, hw, K, x_ld, Cout) of DenseNet-121 at 224 x 224."""
    out = []
    for blk, (c0, n, hw) in enumerate(((64, 6, 56), (128, 12, 28), (256, 24, 14), (512, 16, 7))):
        ld = c0 + 32 * n
        for tag, i in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            out.append((f"block {blk + 1} {tag:6s}", hw, c0 + 32 * i, ld, 128))
        if blk < 3:
            out.append((f"transition {blk + 1}  ", hw, ld, ld, ld // 2))
    return out


def kernels():
    print(f"# kernel A/B, batch {batch}, fp16; us per call (hipGraph replay of 10 calls; median of {reps} alternated rounds of 5 replays, min..max); "
          "GB/s = K input channels + output + filter once")
    g = torch.Generator().manual_seed(0)
    for label, hw, K, ld, Cout in shapes():
        x = torch.randn(batch, hw, hw, ld, generator=g).half().to(dev)
        ps = (0.5 + torch.rand(K, generator=g)).to(dev)
        pt = (0.1 * torch.randn(K, generator=g)).to(dev)
        pk = E.PackedFilter((torch.randn(Cout, K, 1, 1, generator=g) / K ** 0.5).to(dev), torch.float16)
        s2 = (0.5 + torch.rand(Cout, generator=g)).to(dev)
        t2 = (0.1 * torch.randn(Cout, generator=g)).to(dev)
        out = torch.empty(batch, hw, hw, Cout, dtype=torch.float16, device=dev)
        arms = (("preact_conv1x1", True), ("affine_act + conv2d", False))
        graphs = {}
        for k, fused in arms:          # 10 calls of an arm as one hipGraph: the replay times kernels, not the host's enqueue
            def f(fused=fused):
                return E.preact_conv1x1(x, ps, pt, pk, s2, t2, act=E.ACT_RELU, out=out, fused=fused)
            for _ in range(3):
                f()
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
        M = batch * hw * hw
        nbytes = (M * K + M * Cout + Cout * K) * 2
        for k, _ in arms:
            v = sorted(t[k])
            med = v[len(v) // 2]
            print(f"{label} {hw:3d}x{hw:<3d} K={K:4d} ld={ld:4d} Cout={Cout:3d}  {k:20s} {med:8.1f} us ({v[0]:.1f}..{v[-1]:.1f})  {nbytes / med / 1e3:7.0f} GB/s = "
                  f"{nbytes / med / 1e6 / COPY_TBS * 100:5.1f} % of the copy rate", flush=True)
        del x, out, graphs
        torch.cuda.empty_cache()


def model():
    model_on_off("preact", [("DenseNet-121", models.densenet121, 1)], batch, reps, forwards=10, ms_width=7)


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "kernels,model"
    if "kernels" in what:
        kernels()
    if "model" in what:
        model()
