"""Timing of the DBSCAN clustering at the benchmark's scene shape: the 30-fragment synthetic scene's
0.025 m voxel centroids on an index of 0.075 m cells (the index tools/knn_micro.py uses).  mvr_cluster_dbscan
(csrc/dbscan.hip) at eps = 2 and 3 voxels with min_points = 10 on preallocated outputs, and beside it in the same
process mvr_radius_count at the same radius (one walk of the ball: the scale; the clustering makes three and the
hooking).  HIP events around each call after a warm-up, median over --reps calls.  --sklearn adds
sklearn.cluster.DBSCAN over the same fragments on the host's CPUs (one fragment after another, n_jobs = --jobs) as the
CPU baseline and compares the labels.  For the per-kernel split run it once under a kernel trace, e.g.
rocprofv3 --kernel-trace --stats -- python tools/dbscan_micro.py --reps 3
usage: python tools/dbscan_micro.py [--frags 30] [--reps 9] [--min_points 10] [--sklearn [--jobs 16]]"""
import argparse
import os
import sys
import time

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
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=30)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--min_points", type=int, default=10)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--jobs", type=int, default=16)
    a = ap.parse_args()
    frags, _ = synth_scene_fragments(n_frag=a.frags)
    fo = FragmentOverlap(frags, "FCGF", 0.025)
    L = N.lib()
    sizes_b = np.diff(fo.off)
    print("%s: %d fragments of %d..%d centroids (%d in all), cell %.3f m"
          % (N.source_hash(), a.frags, sizes_b.min(), sizes_b.max(), fo.M, fo.r), flush=True)
    labels = torch.empty(fo.M, dtype=torch.int32, device=fo.device)
    sizes = torch.empty(fo.M, dtype=torch.int32, device=fo.device)
    core = torch.empty(fo.M, dtype=torch.uint8, device=fo.device)
    count = torch.empty(fo.M, dtype=torch.int32, device=fo.device)
    n_clusters = torch.empty(fo.B, dtype=torch.int32, device=fo.device)
    ws_b = L.mvr_dbscan_workspace_bytes(fo.M)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=fo.device)
    for voxels in (2, 3):
        eps = voxels * fo.voxel_size

        def cluster():
            N.check(L.mvr_cluster_dbscan(*fo._points(), *fo._fragments(), eps, a.min_points, N.ptr(labels),
                                         N.ptr(n_clusters), N.ptr(sizes), N.ptr(core), N.ptr(ws), ws_b, N.stream()),
                    "mvr_cluster_dbscan")

        def counts():
            N.check(L.mvr_radius_count(*fo._points(), *fo._fragments(), eps, N.ptr(count), N.stream()),
                    "mvr_radius_count")

        t_count = line("mvr_radius_count, radius %.3f (one walk: the scale)" % eps, timed(counts, a.reps))
        t_cluster = line("mvr_cluster_dbscan, eps %.3f, min_points %d, %d points" % (eps, a.min_points, fo.M),
                         timed(cluster, a.reps))
        lab = labels.cpu().numpy()
        print("  %.2f times the count; neighbours %d..%d (mean %.1f); %d core, %d noise, clusters per fragment %d..%d"
              % (t_cluster / t_count, int(count.min()), int(count.max()), float(count.double().mean()),
                 int(core.sum()), int((lab < 0).sum()), int(n_clusters.min()), int(n_clusters.max())), flush=True)
        if a.sklearn:
            from sklearn.cluster import DBSCAN
            xyz = fo.xyz.cpu().numpy()
            t0 = time.perf_counter()
            # a hair under eps: sklearn takes d <= eps, the kernel d < eps
            ref = [DBSCAN(eps=eps * (1.0 - 1e-12), min_samples=a.min_points, n_jobs=a.jobs).fit(
                xyz[fo.off[b]:fo.off[b + 1]]).labels_ for b in range(fo.B)]
            dt = time.perf_counter() - t0
            differ = int((np.concatenate(ref) != lab).sum())
            print("  sklearn DBSCAN per fragment, n_jobs %d: %.1f ms; %d of %d labels differ"
                  % (a.jobs, 1e3 * dt, differ, fo.M), flush=True)


if __name__ == "__main__":
    main()
