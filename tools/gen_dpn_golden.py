"""Generate the DPN fixtures of tests/golden/ — run ONLY in the development container (needs the reference tree, as oracle.gen_golden).

The jobs are built with oracle.gen_golden's own `_fp64` and run by its `main`, so a DPN fixture is made exactly as the fixtures of
oracle.gen_golden.jobs() are: the reference's dpn.py loaded unmodified by path, the model and tests/dpn_restated.py filled from the same
seeded recipe, restatement == reference graph (<= 1e-5, same argmax), then the first seed pair whose top-1 margins exceed 2 x the fp16
bound on every row, whose block states stay below 1000 and whose rows do not share one argmax.

    python tools/gen_dpn_golden.py              # writes the three fixtures
    python tools/gen_dpn_golden.py --check      # writes to a temporary directory and compares with the committed fixtures
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import gen_golden as G  # noqa: E402

PINNED = ("reference-file-on-tlx_cpu (classification/dpn.py unmodified; paddle / paddle2tlx import shims, tlx_MaxPool2d, "
          "tensorlayerx.concat / add / flatten and tensorlayerx.ops.split from the stand-in)")
TAIL = "restatement_max_abs_diff fp16_emulated_err pinned_by param_names param_shapes module_peaks torch_version OUT"


def jobs():
    out = []
    for layers, nc, batch, size, s0, fname in ((68, 1000, 2, (224, 224), 101, "dpn68_b2"), (68, 10, 1, (96, 160), 102, "dpn68_c10_96x160_b1"),
                                               (107, 10, 1, (64, 96), 103, "dpn107_c10_64x96_b1")):
        out.append(G._fp64(fname, "dpn", "dpn", lambda r, a=(layers, nc): r.DPN(layers=a[0], class_num=a[1]),
                           lambda RS, p, x, peaks, layers=layers: RS.dpn(p, x, layers, peaks), batch, size, G.search(s0),
                           dict(arch=f"dpn{layers}", layers=layers, num_classes=nc), PINNED, margins="all", distinct=True,
                           emulate=lambda RS, p, x, rnd, layers=layers: RS.dpn(p, x, layers, None, rnd), tail=TAIL))
    return out


if __name__ == "__main__":
    sys.exit(G.main(sys.argv[1:], todo=jobs()))
