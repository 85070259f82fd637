"""Record what the conv / Linear dispatcher of conv_igemm.hip decides, without a GPU: for a fixed grid of calls print the return
code, tlxmi_last_error() and the tuning flavour's trace lines (TLXMI_TRACE_TILES=1).  Two builds whose outputs are byte-identical
take the same decisions: without a device device_cus() answers 256 (the MI355X's count), the whole cost model runs, and a call ends
at its first launch with TLXMI_ERR_LAUNCH — so the second launch of a tail split is not seen here.  The pointers are fake (16-byte
aligned, never dereferenced on the host), hence the refusal to run where a device would launch on them.
usage: [TLXMI_TUNE_LIB=/path/to/libtlxmi_tune.so] python tools/dispatch_sweep.py > sweep.txt      (a histogram of names goes to stderr)"""
import collections
import ctypes as C
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tlxcv_amd import _lib

X, X2, W, RES, Y, PART = (C.c_void_p(i << 32) for i in range(1, 7))      # 4 GiB apart: no two tensors overlap
SC, SH = C.c_void_p(7 << 32), C.c_void_p((7 << 32) + 65536)
HALF, FULL, BCAST, POOL = _lib.PLAN_SHARED_HALF, _lib.PLAN_SHARED_FULL, 2, _lib.EPI_MAXPOOL_3S2P1
KNOBS = ("TLXMI_TAIL", "TLXMI_PP128", "TLXMI_WREG", "TLXMI_HALO", "TLXMI_PP_DIL", "TLXMI_PLAN_CUS", "TLXMI_TILE", "TLXMI_FORCE", "TLXMI_GCONV",
         "TLXMI_PROJ_TILE", "TLXMI_PROJ_EFF_B")


class Sweep:
    def __init__(self):
        self.lib = _lib._open(_lib.TUNE_LIB_PATH)
        self.log = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        self.calls = 0
        self.names = collections.Counter()
        self.codes = collections.Counter()

    def record(self, label, fn, *args):
        """One call with the library's stderr captured; prints label, return code, error text and the trace lines."""
        sys.stderr.flush()
        os.dup2(self.log.fileno(), 2)
        try:
            rc = fn(*args)
        finally:
            os.dup2(self.saved, 2)
        self.log.seek(0)
        trace = self.log.read().decode()
        self.log.seek(0)
        self.log.truncate()
        err = self.lib.tlxmi_last_error().decode() if rc else ""
        print(f"{label} rc={rc} err={err}")
        sys.stdout.write(trace)
        self.calls += 1
        self.codes[rc] += 1
        self.names.update(re.findall(r"^launched (\S+)", trace, re.M))
        return trace

    def conv(self, label, dt, N, H, Wd, Cin, Cout, k=1, stride=1, pad=0, dil=1, S=None, out_hw=None, res=False, flags=0, act=1, x_ld=0,
             y_ld=0, res_ld=0, y_nstride=0, yoff=0, groups=0, splits=0):
        S = S or k
        Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
        Wo = (Wd + 2 * pad - dil * (S - 1) - 1) // stride + 1
        if out_hw:
            Ho, Wo = out_hw
        d = _lib.ConvDesc(dtype=dt, N=N, H=H, W=Wd, C=Cin, Cout=Cout, R=k, S=S, stride_h=stride, stride_w=stride, pad_h=pad, pad_w=pad,
                          dil_h=dil, dil_w=dil, Ho=Ho, Wo=Wo, x_ld=x_ld or Cin, y_ld=y_ld or Cout, res_ld=(res_ld or Cout) if res else 0,
                          y_nstride=y_nstride, act=act, flags=flags)
        y, r = C.c_void_p(Y.value + yoff), (C.c_void_p(RES.value + yoff) if res else None)
        label = f"{label} dt={dt} {N}x{H}x{Wd}x{Cin}->{Cout} k={k}x{S} s={stride} p={pad} d={dil} res={int(res)} flags={flags:#x} act={act}"
        if splits:
            return self.record(label + f" splits={splits}", self.lib.tlxmi_conv2d_splitk, C.byref(d), splits, X, W, PART, SC, SH, r, y, None)
        if groups:
            return self.record(label + f" groups={groups}", self.lib.tlxmi_group_conv2d, C.byref(d), groups, X, W, SC, SH, r, y, None)
        return self.record(label, self.lib.tlxmi_conv2d, C.byref(d), X, W, SC, SH, r, y, None)

    def probes(self, tag):
        """The shapes that reach every kernel and every split, run under each knob setting."""
        for dt in (0, 1):
            c = lambda *a, **kw: self.conv(tag, dt, *a, **kw)
            c(256, 14, 14, 768, 2304)                                   # ViT-B/16 qkv, proj / fc2, fc1 + GELU
            c(256, 14, 14, 3072, 768, res=True, act=0)
            c(256, 14, 14, 768, 3072, act=6)
            c(64, 14, 14, 512, 2048, act=6, flags=FULL)                 # Swin-B stage 3 at half batch
            c(1, 128, 129, 128, 256)                                    # gemm_wreg: K = 128, K = 256
            c(128, 28, 28, 256, 768)
            c(2, 16, 64, 64, 128, k=3, pad=1)                           # conv_halo
            c(4, 115, 115, 16, 64, k=4, flags=POOL)                     # the pooled stem, Wo = 112
            c(256, 28, 28, 128, 128, k=3, pad=1)                        # ResNet-50 3x3 convs: image-axis tail split at 28 x 28
            c(256, 14, 14, 256, 256, k=3, pad=1)
            c(256, 7, 7, 512, 512, k=3, pad=1)
            c(256, 56, 56, 256, 512, stride=2)                          # strided projection shortcut
            c(256, 56, 56, 64, 256, res=True)
            c(256, 7, 7, 2048, 512)
            c(8, 33, 33, 256, 256, k=3, pad=2, dil=2)                   # dilation 2
            c(2, 15, 13, 64, 264, k=3, S=5, pad=1, out_hw=(15, 11))     # (3, 5) taps
            c(2, 14, 12, 64, 264, k=3, stride=2, out_hw=(7, 6))         # one-sided overhang
            c(1, 9, 31, 256, 291, res=True)                             # Cout % 8 != 0
            c(3, 7, 37, 256, 328, y_ld=376, res=True, res_ld=352, yoff=32)      # column-sliced y / res
            c(3, 1, 50, 256, 256, y_nstride=51 * 256, res=True, flags=BCAST)    # the ViT token matrix
            c(8, 14, 14, 2048, 256, k=3, pad=1, splits=4)               # tlxmi_conv2d_splitk
            c(256, 7, 7, 512, 512, k=3, pad=1, splits=2)
            c(8, 28, 28, 256, 128, k=3, pad=1, splits=2)
            c(8, 28, 28, 256, 256, k=3, pad=1, groups=32)               # block-diagonal chunks (TLXMI_GCONV=0) or the small-group kernel
            self.record(f"{tag} linear_splitk dt={dt}", self.lib.tlxmi_linear_splitk, dt, 256, 25088, 4096, 25088, X, W, 8, PART, SC, SH, None, 0, 1, 0.0,
                        0, Y, 4096, None)
        for (N, Ho, K1, K2, Cout, st) in ((256, 56, 64, 64, 256, 1), (256, 28, 128, 256, 512, 2), (32, 7, 512, 1024, 2048, 2), (3, 14, 256, 512, 1024, 2)):
            H2 = Ho * st
            d = _lib.ProjDesc(dtype=0, N=N, Ho=Ho, Wo=Ho, K1=K1, K2=K2, Cout=Cout, H2=H2, W2=H2, stride=st, x_ld=K1, x2_ld=K2, y_ld=Cout, act=1)
            self.record(f"{tag} proj {N}x{Ho}x{Ho} {K1}+{K2}->{Cout} s={st}", self.lib.tlxmi_conv1x1_proj, C.byref(d), X, X2, W, SH, Y, None)


def main():
    if torch.cuda.is_available():
        sys.exit("dispatch_sweep.py: a GPU is present — the fake pointers would be launched on")
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["TLXMI_TRACE_TILES"] = "1"
    s = Sweep()
    sizes = (64, 128, 256, 512, 1024, 2048)
    for dt in (0, 1):
        for k, pad in ((1, 0), (3, 1)):
            for stride in (1, 2):
                for N in (1, 8, 64, 256):
                    for hw in (7, 14, 28, 56):
                        for Cin in sizes:
                            for Cout in sizes:
                                for flags in (0, HALF, FULL):
                                    for res in (False, True):
                                        s.conv("grid", dt, N, hw, hw, Cin, Cout, k=k, stride=stride, pad=pad, res=res, flags=flags)
    settings = [{}] + [{"TLXMI_TAIL": v} for v in "012"] + [{"TLXMI_PP128": "0"}] + [{"TLXMI_WREG": v} for v in "023"] + [
        {"TLXMI_HALO": "0"}, {"TLXMI_PP_DIL": "0"}, {"TLXMI_PLAN_CUS": "128"}, {"TLXMI_PLAN_CUS": "304"}, {"TLXMI_GCONV": "0"},
        {"TLXMI_PROJ_TILE": "1"}, {"TLXMI_PROJ_TILE": "2"}, {"TLXMI_PROJ_TILE": "3"}, {"TLXMI_PROJ_EFF_B": "0"}, {"TLXMI_FORCE": "50176:768:2304:1:1=9,200704:1152:128:3:1=2"}] + [
        {"TLXMI_TILE": str(v)} for v in range(12)]
    for env in settings:
        os.environ.update(env)
        s.probes(",".join(f"{k}={v}" for k, v in env.items()) or "default")
        for k in env:
            del os.environ[k]
    print(f"# {s.calls} calls; return codes {dict(sorted(s.codes.items()))}", file=sys.stderr)
    for name, n in sorted(s.names.items()):
        print(f"# launched {name:<12} {n}", file=sys.stderr)


if __name__ == "__main__":
    main()
