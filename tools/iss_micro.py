"""Timing and effect of the ISS keypoints (csrc/iss.hip) on the 30-fragment synthetic scene of
tools/fpfh_micro.py: 0.025 m voxel centroids on an index of 0.075 m cells.
--kernels: mvr_iss_saliency beside mvr_estimate_normals at the same radius, and mvr_radius_nms beside mvr_radius_count,
in one process: HIP events per call after a warm-up, the four calls interleaved, median / min / max over --reps.
The threads per workgroup are build-time constants; for 128 and 256 build variants and point MVR_LIB at them:
  tools/build_variant.sh iss.hip iss_t128 -DMVR_ISS_THREADS=128 -DMVR_NMS_THREADS=128
  MVR_LIB=tools/vsp/iss_t128.so python tools/iss_micro.py --kernels
--scene: per non-max radius of --non_max the keypoints per fragment; match_features on all points against
match_keypoints in both modes (host clock around synchronised calls); and the pairs that register_fpfh, its checked
RANSAC and register_fgr bring within 15 degrees / 0.3 m of ground truth (the figure DESIGN.md gives for them) without
keypoints, with match='keypoints' and with match='all'.
usage: python tools/iss_micro.py [--frags 30] [--reps 7] [--kernels] [--scene] [--non_max 0.05 0.035 0.025]"""
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


def event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def kernels(fo, a):
    L = N.lib()
    M, dev = fo.M, fo.device
    normals = torch.empty(M, 3, dtype=torch.float64, device=dev)
    sal = torch.empty(M, dtype=torch.float64, device=dev)
    n_nbr = torch.empty(M, dtype=torch.int32, device=dev)
    keep = torch.empty(M, dtype=torch.uint8, device=dev)
    head = (N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.off_dev), fo.B, M, fo.r)
    nms_r = 2.0 * fo.r / 3.0

    def run_normals():
        assert L.mvr_estimate_normals(*head, fo.r, None, N.ptr(normals), N.ptr(n_nbr), N.stream()) == 0

    def run_saliency():
        assert L.mvr_iss_saliency(*head, fo.r, 0.975, 0.975, 1e-6, 5, N.ptr(sal), N.ptr(n_nbr), N.stream()) == 0

    def run_count(radius):
        assert L.mvr_radius_count(*head, radius, N.ptr(n_nbr), N.stream()) == 0

    def run_nms(radius):
        assert L.mvr_radius_nms(*head, radius, 5, N.ptr(sal), N.ptr(keep), N.stream()) == 0
    runs = [("mvr_estimate_normals, radius %.3f (the scale)" % fo.r, run_normals),
            ("mvr_iss_saliency, radius %.3f" % fo.r, run_saliency),
            ("mvr_radius_count, radius %.3f (the scale)" % fo.r, lambda: run_count(fo.r)),
            ("mvr_radius_nms, radius %.3f" % fo.r, lambda: run_nms(fo.r)),
            ("mvr_radius_count, radius %.3f" % nms_r, lambda: run_count(nms_r)),
            ("mvr_radius_nms, radius %.3f (the default)" % nms_r, lambda: run_nms(nms_r))]
    for _, run in runs:
        run()
    torch.cuda.synchronize()
    ms = [[] for _ in runs]
    for _ in range(a.reps):                      # interleaved: A B C D A B C D ...
        for k, (_, run) in enumerate(runs):
            ms[k].append(event_ms(run))
    for k, (name, _) in enumerate(runs):
        v = sorted(ms[k])
        print("%-50s median %7.3f ms (min %.3f, max %.3f)" % (name, v[len(v) // 2], v[0], v[-1]), flush=True)
    print("  candidates %d of %d points; kept at radius %.3f: %d" % (int((sal > 0).sum()), M, nms_r, int(keep.sum())),
          flush=True)


def within(T, pairs, frags, poses):
    import icp_oracle as O
    ok = 0
    for k, (i, j) in enumerate(pairs):
        D = np.linalg.inv(O.gt_transform(poses, i, j)) @ T[k]
        c = frags[i].astype(np.float64).mean(0)
        ang = np.rad2deg(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
        ok += ang < 15.0 and np.linalg.norm(D[:3, :3] @ c + D[:3, 3] - c) < 0.3
    return ok


def scene(fo, frags, poses, a):
    from lib.fpfh import match_features, match_keypoints, register_fgr, register_fpfh
    xyz = fo.xyz.cpu().numpy()
    fo.estimate_normals(viewpoints=np.asarray([xyz[fo.off[b]:fo.off[b + 1]].mean(0) for b in range(fo.B)]))
    fo.compute_fpfh(fo.r)
    pairs = np.array([(i, j) for i in range(fo.B) for j in range(i + 1, fo.B)], np.int64)
    estimators = (("RANSAC", lambda **kw: register_fpfh(fo, pairs, **kw)),
                  ("checked RANSAC", lambda **kw: register_fpfh(fo, pairs, checkers=True, **kw)),
                  ("FGR", lambda **kw: register_fgr(fo, pairs, **kw)))
    register_fpfh(fo, pairs[:4])
    matches, t_all = clock(lambda: match_features(fo.fpfh, fo.off, pairs))
    counts = np.array([len(m) for m in matches])
    print("match_features on all points, %d pairs: %.1f ms; %d..%d mutual matches (mean %.0f)"
          % (len(pairs), t_all, counts.min(), counts.max(), counts.mean()), flush=True)
    for name, f in estimators:
        out, dt = clock(f)
        print("no keypoints, %s: %d of %d pairs within 15 deg / 0.3 m; %.1f ms end to end"
              % (name, within(out["T"], pairs, frags, poses), len(pairs), dt), flush=True)
    for nms_r in a.non_max:
        kp, t_kp = clock(lambda: fo.iss_keypoints(non_max_radius=nms_r))
        per = np.diff(kp["off"])
        print("non-max radius %.3f: %d candidates, keypoints per fragment %d..%d (median %d, %d in all = %.2f %% of the "
              "points); iss_keypoints %.2f ms" % (nms_r, int((kp["saliency"] > 0).sum()), per.min(), per.max(),
                                                  np.median(per), per.sum(), 100.0 * per.sum() / fo.M, t_kp),
              flush=True)
        for match in ("keypoints", "all"):
            m, t_m = clock(lambda: match_keypoints(fo.fpfh, fo.off, pairs, kp["rows"], kp["off"], True, match))
            c = np.array([len(x) for x in m])
            print("  match=%r: match_keypoints %.1f ms (%.1f x less than all points); %d..%d mutual matches (mean %.1f)"
                  % (match, t_m, t_all / t_m, c.min(), c.max(), c.mean()), flush=True)
            for name, f in estimators:
                out, dt = clock(lambda: f(keypoints=kp, match=match))
                print("  match=%r, %s: %d of %d pairs within 15 deg / 0.3 m; %.1f ms end to end"
                      % (match, name, within(out["T"], pairs, frags, poses), len(pairs), dt), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--scene", action="store_true")
    ap.add_argument("--non_max", type=float, nargs="+", default=[0.05, 0.035, 0.025])
    a = ap.parse_args()
    frags, poses = synth_scene_fragments(n_frag=a.frags)
    fo = FragmentOverlap(frags, "FCGF", 0.025)
    sizes = np.diff(fo.off)
    print("%s: %d fragments of %d..%d centroids (%d in all), cell %.3f m"
          % (N.source_hash(), a.frags, sizes.min(), sizes.max(), fo.M, fo.r), flush=True)
    if a.kernels:
        kernels(fo, a)
    if a.scene:
        scene(fo, frags, poses, a)


if __name__ == "__main__":
    main()
