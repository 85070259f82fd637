"""What binds the bottleneck seam: the launch with parts switched off (tuning flavour, TLXMI_SEAM_DBG bits: 1 no y store,
2 no skip loads, 4 no t1 store, 8 no filter staging after the first step, 16 no MFMAs, 32 no exchange between the waves of a pair
— the wave-pair forms of 256 -> N1 -> 256 know 1, 2, 8, 16, 32).  Timing only — results are garbage.
usage: seam_ablate.py [cases, comma separated] [batch] [TLXMI_SEAM variant] [K1: only the shapes with this many input channels]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tlxcv_amd
from tlxcv_amd import _lib
_lib.tuning().__enter__()
from tlxcv_amd import engine as E

dev = torch.device("cuda:0")
tlxcv_amd.set_precision("fp16")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
os.environ["TLXMI_SEAM"] = sys.argv[3] if len(sys.argv) > 3 else "0"
ONLY = int(sys.argv[4]) if len(sys.argv) > 4 else 0
CASES = [int(v) for v in (sys.argv[1].split(",") if len(sys.argv) > 1 else "0,1,2,4,8,16,3,7,19,23,31".split(","))]
for K1, N1, N2, hw in ((64, 256, 64, 56), (128, 512, 128, 28), (128, 512, 256, 28), (256, 1024, 256, 14)):
    if ONLY and K1 != ONLY:
        continue
    g = torch.Generator().manual_seed(1)
    t2 = torch.randn((B, hw, hw, K1), generator=g).half().to(dev)
    skip = torch.randn((B, hw, hw, N1), generator=g).half().to(dev)
    pk3 = E.PackedFilter((torch.randn((N1, K1, 1, 1), generator=g) * (2 / K1) ** 0.5).to(dev), torch.float16)
    pk1 = E.PackedFilter((torch.randn((N2, N1, 1, 1), generator=g) * (2 / N1) ** 0.5).to(dev), torch.float16)
    s3, h3, s1, h1 = (torch.rand(n, generator=g).to(dev) for n in (N1, N1, N2, N2))
    res = {c: [] for c in CASES}
    for r in range(6):
        for c in CASES:
            os.environ["TLXMI_SEAM_DBG"] = str(c)
            E.bottleneck_seam(t2, pk3, s3, h3, skip, pk1, s1, h1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                E.bottleneck_seam(t2, pk3, s3, h3, skip, pk1, s1, h1)
            e1.record()
            torch.cuda.synchronize()
            res[c].append(e0.elapsed_time(e1) / 5 * 1e3)
    print(f"{K1} -> {N1} -> {N2} @ {hw}: " + "  ".join(f"[{c}] {sorted(v)[len(v) // 2]:.1f}" for c, v in res.items()), flush=True)
