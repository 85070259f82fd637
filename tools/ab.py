"""The measuring code the per-family bench tools (tools/<family>_bench.py) share, on one MI355X: event-timed loops, the hipGraph A/B of
alternated arms, the byte floor of a device-to-device copy, and a model's img/s with an engine option on and off.  What a tool enumerates
(shapes, operands) and what it prints about them stays in the tool; the lines printed here are the `model` sections of
profiles/<family>/*_bench_b256.txt."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tlxcv_amd import _lib, engine as E, seeded  # noqa: E402
from tlxcv_amd.graph import GraphedForward  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us


def _spread(times):
    v = sorted(times)
    return v[len(v) // 2], v[0], v[-1]


def ab(arms, reps):
    """arms: {name: (fn, calls per graph, replays per round[, env of the tuning flavour])} -> {name: (median us per call, min, max)}.
    Each arm is called twice, then captured as one hipGraph of `calls` calls (inside _lib.tuning(**env) where an env is given), so a
    replay times kernels and not the host's enqueue; the arms are alternated for `reps` rounds."""
    graphs = {}
    for k, (f, calls, _, *env) in arms.items():
        def capture():
            for _ in range(2):
                f()
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                for _ in range(calls):
                    f()
            graphs[k].replay()
        if env and env[0] is not None:
            with _lib.tuning(**env[0]):
                capture()
        else:
            capture()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, (_, calls, replays, *_) in arms.items():
            t[k].append(timed(graphs[k].replay, replays) / calls)
    return {k: _spread(t[k]) for k in arms}


def copy_floor(nbytes, calls, reps):
    """(median us, min, max) of a device-to-device copy that moves nbytes in all: nbytes / 2 read and nbytes / 2 written."""
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    return ab({"copy": (lambda: dst.copy_(src), calls, 5)}, reps)["copy"]


def model_on_off(option, variants, batch, reps, forwards=5, ms_width=8):
    """For each (title, factory, seed) of `variants`: the seeded model's forward at 224 x 224 as a hipGraph replay (graph.GraphedForward)
    with the engine option on and off, alternated for `reps` rounds of `forwards` forwards (one count, or an (on, off) pair); prints the
    median ms (min..max) and img/s of either state and the largest logit difference between them."""
    fw = dict(zip((True, False), (forwards, forwards) if isinstance(forwards, int) else forwards))
    how = f"{forwards}" if isinstance(forwards, int) else f"{fw[True]} (on) / {fw[False]} (off)"
    for title, factory, seed in variants:
        m = factory()
        m.load_dict(seeded.fill(seeded.shapes_of(m), seed))
        m = m.to(dev).set_eval()
        x = torch.from_numpy(seeded.image_batch(16, 0)).to(dev).repeat(batch // 16, 1, 1, 1).contiguous()
        graphs = {}
        for on in (True, False):
            E.set_option(option, on)
            with torch.no_grad():
                graphs[on] = GraphedForward(m, x)
        E.set_option(option, True)
        t = {True: [], False: []}
        for _ in range(reps):
            for on in (True, False):
                t[on].append(timed(lambda: graphs[on](), fw[on]))
        print(f"# {title} batch {batch}, 224 x 224, fp16, hipGraph replay; median of {reps} alternated rounds of {how} forwards (min..max)")
        for on in (True, False):
            med, lo, hi = _spread(t[on])
            print(f"{option} {'on ' if on else 'off'}: {med / 1e3:{ms_width}.3f} ms ({lo / 1e3:.3f}..{hi / 1e3:.3f})  {batch / med * 1e6:8.0f} img/s", flush=True)
        d = (graphs[True].static_out.float() - graphs[False].static_out.float()).abs().max().item()
        print(f"max|logit difference| on vs off: {d:.3e}")
        del graphs, m
