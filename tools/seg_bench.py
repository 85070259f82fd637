"""DeepLabV3 (ResNet50_vd, output stride 8) throughput on one MI355X: fp16, 512 x 512, batch 16 by default, eager and as a
hipGraph replay; img/s, ms per step, the analytic FLOPs and the whole-forward rate over the 2.5 PF/s fp16 dense MFMA peak, and
a per-conv-kind table (device events around each conv launch, one forward at a time).  The A/B arm: the same, in the tuning
flavour of the library, with TLXMI_PP_DIL=1 (dilated convs on gemm_pp, the product's choice) and TLXMI_PP_DIL=0 (the generic
implicit-GEMM tiles), alternated.

    python tools/seg_bench.py [--batch 16] [--hw 512] [--steps 20] [--warmup 5] [--out DIR]

--model deeplabv3p: DeepLabV3+ the same way; the per-kind table gets one row per separable conv (fused: one tlxmi_sepconv2d launch;
unfused: the tlxmi_dwconv2d + tlxmi_conv2d pair timed as one), and the A/B arm is the host option "sepconv" on / off (the product
library), alternated --rounds times (default 3 for this model).

    python tools/seg_bench.py --model deeplabv3p [--rounds 3] [--out DIR]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tlxcv_amd  # noqa: E402
from tlxcv_amd import _lib, engine as E, seeded  # noqa: E402
from tlxcv_amd.graph import GraphedForward  # noqa: E402
from tlxcv_amd.models import deeplabv3, deeplabv3p  # noqa: E402

PEAK_FP16 = 2.5e15


def conv_kind(R, dil):
    if R == 1:
        return "1x1"
    return f"3x3 dil{dil}" if dil in (1, 2, 4) else "3x3 dil6-18 (ASPP)"


def time_steps(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def conv_table(m, x, reps=5):
    """Per conv launch: median device time over `reps` forwards, grouped by kind; the dilation is read off the call."""
    orig = E.conv2d
    dils = []

    def rec(x_, pk, stride=1, padding=0, dilation=1, *a, **k):
        dils.append((pk.R, E._pair(dilation)[0]))
        return orig(x_, pk, stride, padding, dilation, *a, **k)
    E.conv2d = rec
    runs = []
    try:
        for _ in range(reps):
            p, dils[:] = [], []
            E.set_probe(p)
            with torch.no_grad():
                m(x)
            torch.cuda.synchronize()
            E.set_probe(None)
            runs.append([(1e3 * e0.elapsed_time(e1), fl) for e0, e1, _, fl, _ in p])
    finally:
        E.conv2d = orig
        E.set_probe(None)
    kinds = {}
    for i, (R, d) in enumerate(dils):
        us = sorted(r[i][0] for r in runs)[reps // 2]
        k = kinds.setdefault(conv_kind(R, d), [0, 0.0, 0.0])
        k[0] += 1
        k[1] += us
        k[2] += runs[0][i][1]
    return {k: {"launches": v[0], "us": round(v[1], 1), "gflop": round(v[2] / 1e9, 2), "tflops": round(v[2] / v[1] / 1e6, 1)}
            for k, v in sorted(kinds.items())}


def sep_table(m, x, reps=5):
    """DeepLabV3+: per launch (median device time over `reps` forwards), the separable convs one row each (in forward order), the other
    convs by kind; the dilation of a plain conv is read off the call as in conv_table()."""
    orig = E.conv2d
    dils = []

    def rec(x_, pk, stride=1, padding=0, dilation=1, *a, **k):
        dils.append((pk.R, E._pair(dilation)[0]))
        return orig(x_, pk, stride, padding, dilation, *a, **k)
    E.conv2d = rec
    runs = []
    try:
        for _ in range(reps):
            p, dils[:] = [], []
            E.set_probe(p)
            with torch.no_grad():
                m(x)
            torch.cuda.synchronize()
            E.set_probe(None)
            runs.append([(1e3 * e0.elapsed_time(e1), fl, shp) for e0, e1, _, fl, shp in p])
    finally:
        E.conv2d = orig
        E.set_probe(None)
    rows, it = {}, iter(dils)
    for i, (_, fl, shp) in enumerate(runs[0]):
        us = sorted(r[i][0] for r in runs)[reps // 2]
        if shp[5] == "sep":
            key = f"sep {shp[3]}->{shp[4]} dil{shp[6]} {'fused' if shp[7] else 'pair'}"
        else:
            key = conv_kind(*next(it))
        k = rows.setdefault(key, [0, 0.0, 0.0])
        k[0] += 1
        k[1] += us
        k[2] += fl
    return {k: {"launches": v[0], "us": round(v[1], 1), "gflop": round(v[2] / 1e9, 2), "tflops": round(v[2] / v[1] / 1e6, 1)}
            for k, v in rows.items()}


def main_v3p(args):
    dev = torch.device("cuda:0")
    tlxcv_amd.set_precision("fp16")
    m = deeplabv3p(num_classes=19)
    m.load_dict(seeded.fill(seeded.shapes_of(m), 1))
    m = m.to(dev).set_eval()
    x = torch.from_numpy(seeded.image_batch(args.batch, 0, hw=args.hw)).to(dev)
    # analytic FLOPs from the probe's shapes: 2 M Cout Cin R S per conv; a separable conv adds its depthwise 2 * 9 * M * C
    p = []
    E.set_probe(p)
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    E.set_probe(None)
    flops = sum(r[3] for r in p)
    res = {"model": "deeplabv3p_resnet50vd_os8", "dtype": "fp16", "batch": args.batch, "hw": args.hw, "conv_launches": len(p),
           "gflop_per_image": round(flops / args.batch / 1e9, 1)}
    arms = {"sepconv=1": True, "sepconv=0": False}
    ab = {k: [] for k in arms}
    tables = {}
    try:
        for _ in range(args.rounds):
            for name, on in arms.items():
                E.set_option("sepconv", on)
                e, g = measure(m, x, args.steps, args.warmup)
                ab[name].append({"eager_ms": round(e, 3), "graph_ms": round(g, 3)})
                tables[name] = sep_table(m, x)
    finally:
        E.set_option("sepconv", True)
    # the kernel at all five (dispatch keeps dilation 1 on the pair): per-launch times of the fused form at the decoder shapes
    orig = E.sepconv2d
    E.sepconv2d = lambda *a, **k: orig(*a, **dict(k, fused=True))
    try:
        tables["fused_all_five"] = {k: v for k, v in sep_table(m, x).items() if k.startswith("sep")}
    finally:
        E.sepconv2d = orig
    graph = sorted(r["graph_ms"] for r in ab["sepconv=1"])[len(ab["sepconv=1"]) // 2]
    res["product"] = {"graph_ms_median": graph, "img_s_graph": round(args.batch / graph * 1e3, 1),
                      "pf_s_graph": round(flops / graph / 1e12, 3), "frac_of_peak_graph": round(flops / graph * 1e3 / PEAK_FP16, 3),
                      "conv_table": tables["sepconv=1"]}
    res["ab_sepconv"] = {k: {"runs": v, "conv_table": tables[k]} for k, v in ab.items()}
    res["sep_fused_all_five"] = tables["fused_all_five"]
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"seg_bench_v3p_b{args.batch}_{args.hw}.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"img_s": res["product"]["img_s_graph"], "ms_per_step": graph, "gflop_per_image": res["gflop_per_image"],
                      "frac_of_peak": res["product"]["frac_of_peak_graph"]}))


def measure(m, x, steps, warmup):
    with torch.no_grad():
        eager = time_steps(lambda: m(x), steps, warmup)
        g = GraphedForward(m, x)
        graph = time_steps(lambda: g(), steps, warmup)
    return eager, graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=None, help="alternations of the A/B arms (2; deeplabv3p: 3)")
    ap.add_argument("--model", default="deeplabv3", choices=("deeplabv3", "deeplabv3p"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "seg_bench needs an MI355X"
    if args.model == "deeplabv3p":
        args.rounds = args.rounds or 3
        return main_v3p(args)
    args.rounds = args.rounds or 2
    dev = torch.device("cuda:0")
    tlxcv_amd.set_precision("fp16")
    m = deeplabv3(num_classes=19)
    m.load_dict(seeded.fill(seeded.shapes_of(m), 1))
    m = m.to(dev).set_eval()
    x = torch.from_numpy(seeded.image_batch(args.batch, 0, hw=args.hw)).to(dev)

    # analytic FLOPs: 2 * M * Cout * Cin * R * S over every conv launch of one forward (from the probe's shapes)
    p = []
    E.set_probe(p)
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    E.set_probe(None)
    flops = sum(r[3] for r in p)
    res = {"model": "deeplabv3_resnet50vd_os8", "dtype": "fp16", "batch": args.batch, "hw": args.hw, "conv_launches": len(p),
           "gflop_per_image": round(flops / args.batch / 1e9, 1)}

    eager, graph = measure(m, x, args.steps, args.warmup)
    res["product"] = {"eager_ms": round(eager, 3), "graph_ms": round(graph, 3), "img_s_graph": round(args.batch / graph * 1e3, 1),
                      "pf_s_graph": round(flops / graph / 1e12, 3), "frac_of_peak_graph": round(flops / graph * 1e3 / PEAK_FP16, 3)}
    res["product"]["conv_table"] = conv_table(m, x)
    print(json.dumps({k: v for k, v in res.items()}, indent=1), flush=True)

    ab = {"1": [], "0": []}
    tables = {}
    for _ in range(args.rounds):
        for arm in ("1", "0"):
            with _lib.tuning(TLXMI_PP_DIL=arm):
                e, g = measure(m, x, args.steps, args.warmup)
                ab[arm].append({"eager_ms": round(e, 3), "graph_ms": round(g, 3)})
                tables[arm] = conv_table(m, x)
    res["ab_pp_dil"] = {f"TLXMI_PP_DIL={k}": {"runs": v, "conv_table": tables[k]} for k, v in ab.items()}
    print(json.dumps(res["ab_pp_dil"], indent=1), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"seg_bench_b{args.batch}_{args.hw}.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"img_s": res["product"]["img_s_graph"], "ms_per_step": res["product"]["graph_ms"],
                      "gflop_per_image": res["gflop_per_image"], "frac_of_peak": res["product"]["frac_of_peak_graph"]}))


if __name__ == "__main__":
    main()
