"""LeViT-128S measurements on one MI355X (fp16).
  shapes: each of the five attention shapes of levit_128s at 224 x 224 — engine.levit_attention on seeded packed rows (the `qkv` rows of a
          stage; q + the `kv` rows of a subsample layer) and a seeded bias grid, Hardswish applied — with the MFMA arm
          (tlxmi_levit_attention) and the plain arm (tlxmi_levit_attention_plain) forced, alternated: `calls` calls of an arm as one
          hipGraph (10 for the MFMA arm, 2 for the plain one, which is not tuned), so the replay times kernels and not the host's
          enqueue.  The MFMA arm is also given in GB/s of its algorithmic bytes (q, k, v read once, out written once, the bias grid
          once: the probe's formula in engine.levit_attention).  A shape keeps the MFMA arm only if its slowest round is faster than the
          plain arm's fastest one (the run-to-run spread printed beside each median).
          The times are hipGraph replay times between two events, NOT the engine probe's per-launch records, which include the host's
          enqueue gap.
  model:  levit_128s img/s as a hipGraph replay (graph.GraphedForward) with "levit_attn" on and off, alternated.
  streams: the same replay at batch, batch / 2 and batch / 4 with the "two_streams" option on and off, alternated: the forward's
          two_streams(128, eager=False) decorator splits a captured batch of >= 128 images into two halves on two streams.
usage: python tools/levit_bench.py [batch=256] [reps=5] [shapes,model,streams]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tlxcv_amd  # noqa: E402,F401
from tlxcv_amd import engine as E, seeded, models  # noqa: E402
from tlxcv_amd.graph import GraphedForward  # noqa: E402
from tools.ab import ab, model_on_off, timed  # noqa: E402

dev = torch.device("cuda:0")
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
# (layers of this shape in levit_128s, Rq, Rk, stride, heads, kd, d)
SHAPES = ((2, 14, 14, 1, 4, 16, 32), (1, 7, 14, 2, 8, 16, 64), (3, 7, 7, 1, 6, 16, 32), (1, 4, 7, 2, 16, 16, 64), (4, 4, 4, 1, 8, 16, 32))


def shapes():
    print(f"# per attention shape of levit_128s at 224 x 224, batch {batch}, fp16; us per call (hipGraph replay; median of {reps} alternated "
          "rounds, min..max)")
    g = torch.Generator().manual_seed(0)
    for n, Rq, Rk, stride, heads, kd, d in SHAPES:
        sub = Rq != Rk
        kv = torch.randn(batch, Rk * Rk, heads * ((kd + d) if sub else (2 * kd + d)), generator=g).half().to(dev)
        q = torch.randn(batch, Rq * Rq, heads * kd, generator=g).half().to(dev) if sub else None
        grid = (torch.randn(heads, Rk, Rk, generator=g) * 0.5).to(dev)
        run = lambda fused: E.levit_attention(kv, grid, heads, kd, d, Rk, kd ** -0.5, q=q, Rq=Rq if sub else None, stride=stride,      # noqa: E731
                                              fused=fused)
        arms = {"mfma": (lambda: run(True), 10, 5), "plain": (lambda: run(False), 2, 2)}
        outs = {k: f() for k, (f, _, _) in arms.items()}
        res = ab(arms, reps)
        nbytes = batch * heads * (Rq * Rq * kd + Rk * Rk * (kd + d) + Rq * Rq * d) * 2 + heads * Rk * Rk * 4
        tag = f"q{Rq}x{Rq} k{Rk}x{Rk} stride {stride} heads {heads:2d} kd {kd} d {d:3d} (x{n})"
        for k, (med, lo, hi) in res.items():
            extra = f"  {nbytes / med / 1e3:7.1f} GB/s" if k == "mfma" else ""
            print(f"{tag} {k:5s} {med:10.1f} us ({lo:.1f}..{hi:.1f}){extra}", flush=True)
        dmax = (outs["mfma"].float() - outs["plain"].float()).abs().max().item()
        keeps = res["mfma"][2] < res["plain"][1]
        print(f"{tag} max|mfma - plain| = {dmax:.3e}, mfma / plain = {res['mfma'][0] / res['plain'][0]:.4f}: "
              f"{'the MFMA arm is faster beyond the spread' if keeps else 'NOT faster beyond the spread: route this shape to the plain arm'}", flush=True)
        del kv, q
        torch.cuda.empty_cache()


def model():
    model_on_off("levit_attn", [("levit_128s", models.levit_128s, 16)], batch, reps, forwards=(10, 4))


def streams():
    m = models.levit_128s()
    m.load_dict(seeded.fill(seeded.shapes_of(m), 16))
    m = m.to(dev).set_eval()
    print(f"# levit_128s, 224 x 224, fp16, hipGraph replay with the two-stream split on and off; median of {reps} alternated rounds of 20 forwards "
          "(min..max)")
    for b in (batch, batch // 2, batch // 4):
        x = torch.from_numpy(seeded.image_batch(16, 0)).to(dev).repeat(b // 16, 1, 1, 1).contiguous()
        graphs = {}
        for on in (True, False):
            E.set_option("two_streams", on)
            with torch.no_grad():
                graphs[on] = GraphedForward(m, x)
        E.set_option("two_streams", True)
        t = {True: [], False: []}
        for _ in range(reps):
            for on in (True, False):
                t[on].append(timed(lambda: graphs[on](), 20))
        for on in (True, False):
            v = sorted(t[on])
            med = v[len(v) // 2]
            print(f"batch {b:4d} two_streams {'on ' if on else 'off'}: {med / 1e3:8.3f} ms ({v[0] / 1e3:.3f}..{v[-1] / 1e3:.3f})  {b / med * 1e6:8.0f} img/s",
                  flush=True)


if __name__ == "__main__":
    what = sys.argv[3] if len(sys.argv) > 3 else "shapes,model,streams"
    if "shapes" in what:
        shapes()
    if "model" in what:
        model()
    if "streams" in what:
        streams()
