"""Timing of scene fusion at the benchmark's scene shape: the 30-fragment synthetic scene's 0.025 m
voxel centroids (about 612 k points, the index tools/icp_micro.py and tools/fpfh_micro.py time on) under their
ground-truth poses.  mvr_fuse_scene (csrc/fuse.hip) at 0.025 m and 0.05 m, with and without normals, and in the same
run mvr_voxel_centroids (csrc/overlap.hip) over the same number of points (the centroids as fp32 input, the same
fragment offsets): the nearest launch sequence the library had before, key + 7-pass sort + scan + one thread per run
with runs of one or two points.  HIP events around windows of 20 calls after a warm-up, alternating the cases, median
over --reps windows; effective bytes per second against the bytes the launches must move (counted below from the
shapes); a checksum of the rows, to compare builds.
usage: python tools/fuse_micro.py [--frags 30] [--reps 21] [--voxel 0.025 0.05]"""
import argparse
import hashlib
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


def fuse_bytes(M, V, normals):
    """per point: transform 24 + 28 (+ 24 + 24 with normals), keys 28 + 20, histogram 8, 8 sort passes of 12 + 12,
    sorted keys 20, head flags 12, scan 12, run starts 8, the run's gathers 32 (+ 24); per voxel: its start 4 and its
    row 32 (+ 24)"""
    extra = 24 if normals else 0
    return M * (52 + 48 + 8 + 8 * 24 + 20 + 12 + 12 + 8 + 32 + 3 * extra) + V * (36 + extra)


def centroid_bytes(M, V, passes):
    """per point: minimum 12, keys 12 + 20, histogram 8, sort passes of 24, sorted keys 20, head flags 12, scan 12,
    the run's reads 28; per voxel: its row 24"""
    return M * (12 + 32 + 8 + passes * 24 + 20 + 12 + 12 + 28) + V * 24


INNER = 20      # calls between a pair of events: a window of several milliseconds, not one 0.3 ms call


def event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / INNER


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=30)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--voxel", type=float, nargs="+", default=[0.025, 0.05], help="voxel sizes of the fusion")
    a = ap.parse_args()
    frags, poses = synth_scene_fragments(n_frag=a.frags)
    fo = FragmentOverlap(frags, "FCGF", 0.025)
    xyz = fo.xyz.cpu().numpy()
    fo.estimate_normals(viewpoints=np.asarray([xyz[fo.off[b]:fo.off[b + 1]].mean(0) for b in range(fo.B)]))
    dev, M, B = fo.device, fo.M, fo.B
    L = N.lib()
    g_poses = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, np.float64)[:, :3, :]).reshape(B, 12)).to(dev)
    out_xyz, out_nrm = (torch.empty(M, 3, dtype=torch.float64, device=dev) for _ in range(2))
    n_points, n_frags = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(2))
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws_b = L.mvr_fuse_scene_workspace_bytes(M)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
    s = N.stream()

    def fuse(voxel, normals):
        N.check(L.mvr_fuse_scene(N.ptr(fo.xyz), N.ptr(fo.normals) if normals else None, N.ptr(fo.off_dev), B, M,
                                 N.ptr(g_poses), None, voxel, N.ptr(ws), ws_b, N.ptr(out_xyz),
                                 N.ptr(out_nrm) if normals else None, N.ptr(n_points), N.ptr(n_frags), N.ptr(count),
                                 s), "mvr_fuse_scene")

    x32 = fo.xyz.to(torch.float32).contiguous()
    cws_b = L.mvr_voxel_centroids_workspace_bytes(M)
    cws = torch.empty(cws_b, dtype=torch.uint8, device=dev)
    c_out = torch.empty(M, 3, dtype=torch.float64, device=dev)
    c_off = torch.empty(B + 1, dtype=torch.int64, device=dev)

    def centroids():
        N.check(L.mvr_voxel_centroids(N.ptr(x32), N.ptr(fo.off_dev), B, M, 0.025, N.ptr(cws), cws_b, N.ptr(c_out),
                                      N.ptr(c_off), s), "mvr_voxel_centroids")

    cases = []
    for v in a.voxel:
        cases += [("mvr_fuse_scene, voxel %g, normals" % v, lambda v=v: fuse(v, True)),
                  ("mvr_fuse_scene, voxel %g" % v, lambda v=v: fuse(v, False))]
    cases.append(("mvr_voxel_centroids, voxel 0.025", centroids))
    info = []
    for name, run in cases:                       # warm-up of every shape, and the shapes' voxel counts
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        if run is centroids:
            V = int(c_off[-1].item())
            info.append((V, centroid_bytes(M, V, (48 + max(1, (B - 1).bit_length()) + 7) // 8), None, None, None))
        else:
            V = int(count.item())
            nf, npts = n_frags[:V], n_points[:V]
            h = hashlib.sha256()
            for x in (out_xyz[:V], nf, npts) + ((out_nrm[:V],) if "normals" in name else ()):
                h.update(x.cpu().numpy().tobytes())
            info.append((V, fuse_bytes(M, V, "normals" in name), int(npts.max().item()),
                         float((nf >= 2).double().mean().item()), h.hexdigest()[:12]))
    ms = [[] for _ in cases]
    for _ in range(a.reps):                       # alternating: other work on the machine hits every case alike
        for k, (_, run) in enumerate(cases):
            ms[k].append(event_ms(run))
    print("%s: %d fragments, %d points" % (N.source_hash(), B, M), flush=True)
    for (name, _), t, (V, nbytes, longest, shared, digest) in zip(cases, ms, info):
        t.sort()
        med = t[len(t) // 2]
        runs = "%.2f points per run" % (M / max(V, 1))
        if longest is not None:
            runs += ", longest %d, %.0f%% seen by two or more fragments, rows sha256 %s" % (longest, 100 * shared,
                                                                                             digest)
        print("%s: median %.3f ms (min %.3f, max %.3f) over %d windows of %d calls; %d voxels (%s); %.1f MB to move "
              "-> %.0f GB/s effective" % (name, med, t[0], t[-1], len(t), INNER, V, runs, nbytes / 1e6,
                                          nbytes / med * 1e-6), flush=True)


if __name__ == "__main__":
    main()
