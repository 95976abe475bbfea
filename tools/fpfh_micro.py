"""Timing of the weights-free coarse registration at the benchmark's scene shape: the 30-fragment
synthetic scene's 0.025 m voxel centroids (the index tools/icp_micro.py times the normals and the ICPs on) and its 435
pairs.  mvr_compute_fpfh (csrc/fpfh.hip) at radius = the cell (0.075 m) on normals oriented to the fragments' means,
mvr_feat_match (csrc/feat_match.hip) for the 435 pairs in both directions, and lib.fpfh.register_fpfh end to end
(both matcher launches, the mutual filter and the padding in torch, mvr_ransac), with the share of pairs it registers
within 15 degrees / 0.3 m of ground truth.  HIP events around each call after a warm-up, median over --reps calls;
register_fpfh by the host clock around a synchronised call.  --demo also registers tests/golden/demo's pair.
--checkers repeats the register_fpfh lines with checkers=True (mvr_ransac_checked) and prints how many
of its 100000 samples per pair passed the checkers and how many were scored.
usage: python tools/fpfh_micro.py [--frags 30] [--reps 5] [--demo] [--checkers]"""
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
from lib.fpfh import feat_match, register_fpfh  # noqa: E402
from lib.overlap import FragmentOverlap  # noqa: E402
import icp_oracle as O  # noqa: E402
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


def oriented(fo):
    xyz = fo.xyz.cpu().numpy()
    fo.estimate_normals(viewpoints=np.asarray([xyz[fo.off[b]:fo.off[b + 1]].mean(0) for b in range(fo.B)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--demo", action="store_true")
    ap.add_argument("--checkers", action="store_true")
    a = ap.parse_args()
    frags, poses = synth_scene_fragments(n_frag=a.frags)
    fo = FragmentOverlap(frags, "FCGF", 0.025)
    oriented(fo)
    sizes = np.diff(fo.off)
    pairs = np.array([(i, j) for i in range(a.frags) for j in range(i + 1, a.frags)], np.int64)
    both = np.concatenate([pairs, pairs[:, ::-1]])
    print("%s: %d fragments of %d..%d centroids (%d in all), %d pairs, cell %.3f m, neighbours %d..%d (mean %.1f)"
          % (N.source_hash(), a.frags, sizes.min(), sizes.max(), fo.M, len(pairs), fo.r, int(fo.n_nbr.min()),
             int(fo.n_nbr.max()), float(fo.n_nbr.double().mean())), flush=True)
    ms = timed(lambda: fo.compute_fpfh(fo.r), a.reps)
    nb = float(fo.n_nbr.double().sum()) - fo.M            # neighbours without the point itself
    print("mvr_compute_fpfh, %d points, radius %.3f: median %.3f ms (min %.3f, max %.3f); %.3g neighbour visits per "
          "pass, %.3g bytes of SPFH rows read by the second pass" % (fo.M, fo.r, ms[len(ms) // 2], ms[0], ms[-1], nb,
                                                                    nb * 33 * 8), flush=True)
    F = fo.fpfh
    flop = 2.0 * 33 * float((sizes[both[:, 0]] * sizes[both[:, 1]]).sum())
    ms = timed(lambda: feat_match(F, fo.off, both), max(2, a.reps // 2))
    print("mvr_feat_match, %d pairs x 2 directions, C = 33: median %.1f ms (min %.1f, max %.1f); 2 C n_q n_t = %.3g "
          "FLOP -> %.1f TFLOP/s" % (len(pairs), ms[len(ms) // 2], ms[0], ms[-1], flop, flop / ms[len(ms) // 2] * 1e-9),
          flush=True)
    for checkers in (False, True)[:1 + a.checkers]:
        register_fpfh(fo, pairs[:4], checkers=checkers)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = register_fpfh(fo, pairs, checkers=checkers)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ok = 0
        for k, (i, j) in enumerate(pairs):
            Tg = O.gt_transform(poses, i, j)
            c = frags[i].astype(np.float64).mean(0)
            D = np.linalg.inv(Tg) @ out["T"][k]
            ang = np.rad2deg(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
            ok += ang < 15.0 and np.linalg.norm(D[:3, :3] @ c + D[:3, 3] - c) < 0.3
        print("register_fpfh%s, %d pairs end to end: %.1f ms; mutual matches %d..%d (mean %.0f); %d pairs within "
              "15 deg / 0.3 m of ground truth" % ("(checkers=True)" if checkers else "", len(pairs), dt * 1e3,
                                                  out["n_matches"].min(), out["n_matches"].max(),
                                                  out["n_matches"].mean(), ok), flush=True)
        if checkers:
            print("  samples passing the checkers per pair: %d..%d (median %d, mean %.0f) of 100000; scored: %d..%d "
                  "(median %d, mean %.0f)" % (out["n_pass"].min(), out["n_pass"].max(), np.median(out["n_pass"]),
                                             out["n_pass"].mean(), out["n_valid"].min(), out["n_valid"].max(),
                                             np.median(out["n_valid"]), out["n_valid"].mean()), flush=True)
    if a.demo:
        from lib.ply import read_ply_xyz
        demo = os.path.join(ROOT, "tests", "golden", "demo")
        raw = [read_ply_xyz(os.path.join(demo, "cloud_bin_%d.ply" % k)) for k in range(2)]
        fd = FragmentOverlap(raw, "FCGF", 0.025, radius=0.125)
        xyz = fd.xyz.cpu().numpy()
        fd.estimate_normals(0.05, viewpoints=np.asarray([xyz[fd.off[b]:fd.off[b + 1]].mean(0) for b in range(2)]))
        fd.compute_fpfh(0.125)
        r = register_fpfh(fd, [[0, 1]])
        print("demo pair (%d / %d centroids, FPFH radius 0.125, normals 0.05): %d mutual matches, RANSAC fitness %.4f, "
              "rmse %.4f" % (fd.off[1], fd.off[2] - fd.off[1], r["n_matches"][0], r["fitness"][0], r["rmse"][0]))
        from lib.icp import icp_refine
        ref = icp_refine(fd, [[0, 1]], r["T"], max_dist=0.05)
        print("  after icp_refine (max_dist 0.05): fitness %.4f, rmse %.4f, %d iterations"
              % (ref["fitness"][0], ref["rmse"][0], ref["iters"][0]))
        if a.checkers:
            rc = register_fpfh(fd, [[0, 1]], checkers=True)
            refc = icp_refine(fd, [[0, 1]], rc["T"], max_dist=0.05)
            D = np.linalg.inv(r["T"][0]) @ rc["T"][0]
            print("demo pair, checkers=True: %d of 100000 samples passed, %d scored, RANSAC fitness %.4f, rmse %.4f; "
                  "after icp_refine fitness %.4f, rmse %.4f; %.2f deg / %.3f m from the plain estimate"
                  % (rc["n_pass"][0], rc["n_valid"][0], rc["fitness"][0], rc["rmse"][0], refc["fitness"][0],
                     refc["rmse"][0], np.rad2deg(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1))),
                     np.linalg.norm(D[:3, 3])))


if __name__ == "__main__":
    main()
