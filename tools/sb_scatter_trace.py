"""Phase times of level-1 binning's scatter (sb_scatter) per workgroup on the bench frame, from a
GSR_SB_TRACE build (global sort, so that the local sort's stamps do not share the slots):
    python3 street-sparse-3dgs_amd/build_hip.py --define GSR_SB_TRACE=1 --out vlibs/sbtrace.so
    GSR_LIBRARY=vlibs/sbtrace.so python3 tools/sb_scatter_trace.py
Stamps of wave 0: 0 start (loads issued), 1-3 mark / prefix / write of round 0, 4-6 of round 1, 7 end.
Prints the median / p90 / max of every interval between consecutive stamps (us) and the kernel span."""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "street-sparse-3dgs_amd"))
import bench  # noqa: E402

NAMES = sys.argv[1].split(",") if len(sys.argv) > 1 else ["init + mark 0", "wait + prefix 0", "wait + write 0",
                                                           "clear + mark 1", "wait + prefix 1", "wait + write 1", "end"]


def main():
    import torch
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    W, H = 1920, 1080
    s, inp, gcol, ginv = bench.make_inputs(1_000_000, W, H, 3, 0, dev)
    rs, raster = bench.rasterizer_for(s, W, H, 3, dev)
    step = bench.fwd_bwd_step(raster, inp, gcol, ginv)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    buf = (ctypes.c_int64 * (2048 * 8))()
    _C._L.gsr_debug_trace(buf, 2048 * 8, 1)
    step()
    torch.cuda.synchronize()
    _C._L.gsr_debug_trace(buf, 2048 * 8, 0)
    a = np.array(buf[:], np.int64).reshape(2048, 8)
    a = a[(a > 0).all(axis=1)]  # workgroups that ran both rounds
    t0 = a[:, 0].min()
    print("workgroups", len(a), "kernel span us", (a[:, 7].max() - t0) / 100.0)
    print("start offsets us: median %.1f p90 %.1f max %.1f" % tuple(np.percentile((a[:, 0] - t0) / 100.0, [50, 90, 100])))
    for i, nme in enumerate(NAMES):
        d = (a[:, i + 1] - a[:, i]) / 100.0
        print(f"{nme:18s} median {np.median(d):7.2f} p90 {np.percentile(d, 90):7.2f} max {d.max():7.2f} us")
    tot = (a[:, 7] - a[:, 0]) / 100.0
    print(f"{'total':18s} median {np.median(tot):7.2f} p90 {np.percentile(tot, 90):7.2f} max {tot.max():7.2f} us")


if __name__ == "__main__":
    main()
