"""Timing of the exact k-nearest-neighbour search and the outlier filters at the benchmark's scene
shape: the 30-fragment synthetic scene's 0.025 m voxel centroids on an index of 0.075 m cells (the index
tools/icp_micro.py and tools/fpfh_micro.py use).  mvr_knn_self (csrc/knn_self.hip) at k = 20 and k = 64 with the share
of queries its second launch (the direct scan) resolved, FragmentOverlap.statistical_outliers (the search, the
statistics and the mask), radius_outliers, and on the same index in the same run estimate_normals as the scale and a
per-fragment torch.cdist + topk brute force as the comparator (fp64, as the kernel).  HIP events around each call after
a warm-up, median over --reps calls.  --check compares the kernel's neighbours with the brute force's on every
fragment (squared distances to 1e-12 relative: cdist rounds otherwise).
The last ring the first launch walks is a build-time constant; for 3 instead of 2 build a variant and point MVR_LIB
at it:  tools/build_variant.sh knn_self.hip knn_rho3 -DMVR_KNN_RHO_MAX=3;  MVR_LIB=tools/vsp/knn_rho3.so python ...
usage: python tools/knn_micro.py [--frags 30] [--reps 5] [--check]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d_multiview_reg_amd"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lib import _native as N  # noqa: E402
from lib.overlap import FragmentOverlap  # noqa: E402
from synth import synth_scene_fragments  # noqa: E402


def timed(run, reps):
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms


def line(what, ms):
    print("%s: median %.3f ms (min %.3f, max %.3f)" % (what, ms[len(ms) // 2], ms[0], ms[-1]), flush=True)


def scanned(fo):
    """the queries the last mvr_knn_self on this stream left to its second launch (the workspace's first word)"""
    ws = N.workspace(N.lib().mvr_knn_self_workspace_bytes(fo.M), fo.device)
    return int(ws[:4].view(torch.int32).item())


def brute(fo, k):
    """per fragment: all squared distances by torch.cdist, the k smallest by topk"""
    out = []
    for b in range(fo.B):
        x = fo.xyz[fo.off[b]:fo.off[b + 1]]
        d = torch.cdist(x, x)
        out.append(torch.topk(d, min(k, len(x)), dim=1, largest=False))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    frags, _ = synth_scene_fragments(n_frag=a.frags)
    fo = FragmentOverlap(frags, "FCGF", 0.025)
    sizes = np.diff(fo.off)
    print("%s: %d fragments of %d..%d centroids (%d in all), cell %.3f m"
          % (N.source_hash(), a.frags, sizes.min(), sizes.max(), fo.M, fo.r), flush=True)
    line("estimate_normals, radius %.3f (the scale)" % fo.r, timed(lambda: fo.estimate_normals(), a.reps))
    print("  neighbours within the cell size: %d..%d (mean %.1f)"
          % (int(fo.n_nbr.min()), int(fo.n_nbr.max()), float(fo.n_nbr.double().mean())), flush=True)
    for k in (20, 64):
        ms = timed(lambda: fo.knn(k), a.reps)
        n = scanned(fo)
        line("mvr_knn_self, k = %d, %d points" % (k, fo.M), ms)
        print("  %d queries (%.4f %%) went to the direct scan" % (n, 100.0 * n / fo.M), flush=True)
    line("statistical_outliers(20, 2.0): the search, the statistics, the mask",
         timed(lambda: fo.statistical_outliers(20, 2.0), a.reps))
    st = fo.statistical_outliers(20, 2.0)
    print("  %d of %d points removed" % (int((~st["keep"]).sum()), fo.M), flush=True)
    line("radius_outliers(16, %.3f)" % fo.r, timed(lambda: fo.radius_outliers(16), a.reps))
    for k in (20, 64):
        line("torch.cdist + topk per fragment, k = %d (the comparator)" % k, timed(lambda: brute(fo, k), a.reps))
    if a.check:
        idx, d2 = fo.knn(20)
        worst = 0.0
        for b, (val, _) in enumerate(brute(fo, 20)):
            mine = d2[fo.off[b]:fo.off[b + 1]].sqrt()
            worst = max(worst, float(((mine - val).abs() / val.clamp_min(1e-30))[:, 1:].max()))
        print("check: k-th distances against the brute force, largest relative difference %.3g" % worst)


if __name__ == "__main__":
    main()
