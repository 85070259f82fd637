"""Generate the ReXNet fixtures of tests/golden/ — run ONLY in the development container (needs the reference tree, as oracle.gen_golden).

The jobs are built with oracle.gen_golden's own `_fp64` and run by its `main`, so a ReXNet fixture is made exactly as the fixtures of
oracle.gen_golden.jobs() are: the reference's rexnet.py loaded unmodified by path, the model and tests/rexnet_restated.py filled from the
same seeded recipe, restatement == reference graph (<= 1e-5, same argmax), then the first seed pair whose top-1 margins exceed 2 x the fp16
bound on every row and whose block outputs stay below 1000.

The rows of a batch may share one argmax, so `distinct` is off; instead this tool requires the two rows of the batch-2 fixture to differ
by more than 2 x the bound somewhere, so that a row mix-up cannot pass the GPU test.

    python tools/gen_rexnet_golden.py              # writes the four fixtures
    python tools/gen_rexnet_golden.py --check      # writes to a temporary directory and compares with the committed fixtures
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import gen_golden as G  # noqa: E402

PINNED = "reference-file-on-tlx_cpu (classification/rexnet.py unmodified; paddle / paddle2tlx import shims and tlx_Dropout from the stand-in)"
TAIL = "restatement_max_abs_diff fp16_emulated_err pinned_by param_names param_shapes module_peaks torch_version OUT"


def jobs():
    out = []
    for arch, wm, nc, batch, size, s0, fname in (("rexnet_1_0", 1.0, 1000, 2, (224, 224), 121, "rexnet_1_0_b2"),
                                                  ("rexnet_1_3", 1.3, 10, 1, (96, 160), 122, "rexnet_1_3_c10_96x160_b1"),
                                                  ("rexnet_1_5", 1.5, 10, 1, (96, 160), 123, "rexnet_1_5_c10_96x160_b1"),
                                                  ("rexnet_2_0", 2.0, 10, 1, (64, 96), 124, "rexnet_2_0_c10_64x96_b1")):
        out.append(G._fp64(fname, "rexnet", "rexnet", lambda r, a=(arch, nc): getattr(r, a[0])(class_num=a[1]),
                           lambda RS, p, x, peaks, w=wm: RS.rexnet(p, x, w, peaks), batch, size, G.search(s0),
                           dict(arch=arch, width_mult=wm, num_classes=nc), PINNED, margins="all", distinct=False,
                           emulate=lambda RS, p, x, rnd, w=wm: RS.rexnet(p, x, w, None, rnd), tail=TAIL))
    return out


def rows_differ(path):
    """The batch-2 fixture: its two rows of logits differ by more than 2 x the fp16 bound somewhere."""
    g = np.load(path)
    lg = g["logits"]
    bound = max(0.003 * float(lg.max() - lg.min()), 3 * float(g["fp16_emulated_err"]))
    d = float(np.abs(lg[0] - lg[1]).max())
    print(f"{os.path.basename(path)}: max|row 0 - row 1| = {d:.4f}, 2 x the bound = {2 * bound:.4f}")
    assert lg.shape[0] == 2 and d > 2 * bound, "the rows of the batch-2 fixture are too close: a row mix-up could pass"


if __name__ == "__main__":
    rc = G.main(sys.argv[1:], todo=jobs())
    b2 = os.path.join(G.GOLDEN, "rexnet_1_0_b2.npz")
    if os.path.isfile(b2):
        rows_differ(b2)
    sys.exit(rc)
