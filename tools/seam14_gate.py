"""The gate of the 14 x 14 seams (resnet.SEAM14_IMAGES: images per launch between which 256 -> 1024 -> 256 runs as one fused launch),
re-measured with the gate open: ResNet-50 fp16 on the hipGraph replay, per batch the forward with the 14 x 14 seams fused and with them as
two launches (option "seam256" off), interleaved, median of 5.  Forwards of >= 96 images run as two half batches on two streams, so a
launch sees half the batch there.   usage: seam14_gate.py [batches]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402
from tlxcv_amd import seeded, models, engine as E  # noqa: E402
from tlxcv_amd.graph import GraphedForward  # noqa: E402
from tlxcv_amd.models.classification import resnet  # noqa: E402

dev = torch.device("cuda:0")
tlxcv_amd.set_precision("fp16")
gate = resnet.SEAM14_IMAGES
resnet.SEAM14_IMAGES = (12, 1 << 30)
batches = [int(v) for v in (sys.argv[1].split(",") if len(sys.argv) > 1 else "32,64,96,128,192,256,384,512".split(","))]
m = models.resnet50()
m.load_dict(seeded.fill(seeded.shapes_of(m), 1))
m = m.to(dev).set_eval()
print(f"== resnet50 fp16, hipGraph replay, gate open (product gate: {gate[0]} .. {gate[1]} images a launch); ms per forward", flush=True)
for bs in batches:
    x = torch.from_numpy(seeded.image_batch(min(bs, 16), 0)).to(dev).repeat((bs + 15) // 16, 1, 1, 1)[:bs].half().contiguous()
    graphs = {"fused": GraphedForward(m, x)}
    E.set_option("seam256", 0)
    try:
        graphs["two launches"] = GraphedForward(m, x)
    finally:
        E.set_option("seam256", 1)
    ts = {k: [] for k in graphs}
    for r in range(5):
        for k, f in graphs.items():
            f(); torch.cuda.synchronize()
            n = 20 if bs <= 128 else 10
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            torch.cuda.synchronize()
            ts[k].append(1e3 * (time.perf_counter() - t0) / n)
    med = {k: sorted(v)[2] for k, v in ts.items()}
    per = bs // 2 if bs >= 96 else bs
    print(f"batch {bs:4d} ({per:3d} a launch, {'inside' if gate[0] <= per <= gate[1] else 'outside'} the product gate): fused {med['fused']:.3f} ms   "
          f"two launches {med['two launches']:.3f} ms   fused is {100 * (med['two launches'] - med['fused']) / med['two launches']:+.1f} % faster", flush=True)
    del graphs
