"""The oracle's distance from fp64 autograd on the scenes of tests/test_gpu_shapes.py, per tensor and
claimed subset: the records (kind oracle_vs_fp64, case gpu_<name>) that the GPU bars of that file are
stated against.  CPU only; the 3000-row frames take minutes in fp64 (dense_torch.dense_grads with
per_tile=True), which is why they are recorded here and not measured inside a test.

    GSR_SHAPE_RECORD=profiles/r12_shape_margins.jsonl python tools/shape_yardstick.py [case ...]
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), os.path.join(REPO, "street-sparse-3dgs_amd")]

import dense_torch as DT  # noqa: E402
import shape_cases as SC  # noqa: E402
import test_gpu_shapes as T  # noqa: E402
from helpers import rel_l2  # noqa: E402
from test_oracle import FP64_PAIRS  # noqa: E402


def main(names):
    for c in T.CASES:
        if names and c["name"] not in names:
            continue
        t0 = time.time()
        s, dcol, dinv, st, g, sub = T.reference(c["name"])
        d = DT.dense_grads(st, dcol, dinv, per_tile=True)
        err = dict(color=rel_l2(st["color"], d["color"]), invdepth=rel_l2(st["invdepth"], d["invdepth"]))
        for dk, ok in FP64_PAIRS:
            got, ref = g[ok].reshape(d[dk].shape), d[dk]
            err[ok] = rel_l2(got, ref)
            for n, m in sub.items():
                err[f"{ok}@{n}"] = rel_l2(got[m], ref[m])
        SC.record("oracle_vs_fp64", "gpu_" + c["name"], **err)
        print(c["name"], f"{time.time() - t0:.0f} s", {k: f"{v:.1e}" for k, v in err.items()}, flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
