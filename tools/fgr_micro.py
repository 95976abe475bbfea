"""Timing of Fast Global Registration (csrc/fgr.hip mvr_fgr) beside the two RANSACs on the same
correspondences, in one process: 435 pairs of tests/ransac_checked_oracle.corr(2000, 0.3, seed) (30 % planted inliers,
5 mm noise).  mvr_fgr at its defaults (tuple filter on; and off), mvr_ransac at 4-point / 2500 iterations and
mvr_ransac_checked at its defaults: HIP events per call after a warm-up, median / min / max over --reps, the calls
interleaved, and how many pairs each brings within 1 degree / 0.02 m of the planted motion.
--scene: lib.fpfh.register_fgr on the 30-fragment synthetic scene of tools/fpfh_micro.py, its wall time (host clock
around synchronised calls) split into match_features, the Python gather of correspondences and run_fgr_batch, and the
pairs within 15 degrees / 0.3 m of ground truth (the figure DESIGN.md gives for the RANSACs).
usage: python tools/fgr_micro.py [--pairs 435] [--n 2000] [--inliers 0.3] [--reps 7] [--scene]"""
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
from ransac_checked_oracle import corr  # noqa: E402


def event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def recovered(T, truth, deg=1.0, metres=0.02):
    ok = 0
    for k, (R, t) in enumerate(truth):
        c = np.clip((np.trace(T[k, :3, :3].T @ R) - 1.0) / 2.0, -1.0, 1.0)
        ok += np.rad2deg(np.arccos(c)) < deg and np.linalg.norm(T[k, :3, 3] - t) < metres
    return ok


def launches(a):
    d = torch.device("cuda")
    data = [corr(a.n, a.inliers, seed=p) for p in range(a.pairs)]
    x1 = torch.from_numpy(np.stack([c[0] for c in data])).to(d)
    x2 = torch.from_numpy(np.stack([c[1] for c in data])).to(d)
    truth = [(c[2], c[3]) for c in data]
    P, n = a.pairs, a.n
    cnt = torch.full((P,), n, dtype=torch.int32, device=d)
    T = torch.empty(P, 4, 4, dtype=torch.float64, device=d)
    fit, rmse = (torch.empty(P, dtype=torch.float64, device=d) for _ in range(2))
    i32 = [torch.empty(P, dtype=torch.int32, device=d) for _ in range(3)]
    L = N.lib()
    ws = torch.empty(max(L.mvr_fgr_workspace_bytes(P, n, 1000), L.mvr_ransac_workspace_bytes(P, 2500),
                         L.mvr_ransac_checked_workspace_bytes(P, 100000, 2500)), dtype=torch.uint8, device=d)

    def fgr(tuple_factor):
        assert L.mvr_fgr(N.ptr(x1), N.ptr(x2), 3 * n, N.ptr(cnt), P, 0.05, 64, 1.4, tuple_factor, 1000, 0.95, 0,
                         N.ptr(T), N.ptr(fit), N.ptr(rmse), N.ptr(i32[0]), N.ptr(i32[1]), N.ptr(i32[2]), None,
                         N.ptr(ws), ws.numel(), N.stream()) == 0

    def ransac():
        assert L.mvr_ransac(N.ptr(x1), N.ptr(x2), 3 * n, N.ptr(cnt), P, 4, 2500, 0.05, 0, N.ptr(T), N.ptr(fit),
                            N.ptr(rmse), N.ptr(i32[0]), None, N.ptr(ws), ws.numel(), N.stream()) == 0

    def checked():
        assert L.mvr_ransac_checked(N.ptr(x1), N.ptr(x2), 3 * n, N.ptr(cnt), P, 3, 100000, 0.05, 0, 2500, 0.9, 0.05,
                                    None, None, -1.0, N.ptr(T), N.ptr(fit), N.ptr(rmse), N.ptr(i32[0]),
                                    N.ptr(i32[1]), N.ptr(i32[2]), None, None, None, N.ptr(ws), ws.numel(),
                                    N.stream()) == 0
    runs = [("mvr_fgr, tuple filter on (100 n tests, 1000 tuples, 64 iterations)", lambda: fgr(100)),
            ("mvr_fgr, tuple filter off (all rows, 64 iterations)", lambda: fgr(0)),
            ("mvr_ransac, 4-point, 2500 iterations", ransac),
            ("mvr_ransac_checked, 3-point, 100000 draws, cap 2500", checked)]
    print("%s: %d pairs x %d correspondences, %.0f %% inliers" % (N.source_hash(), P, n, 100 * a.inliers), flush=True)
    notes = []
    for name, run in runs:                       # warm-up, and what each one recovers
        run()
        torch.cuda.synchronize()
        note = "%d of %d pairs within 1 deg / 0.02 m, mean fitness %.3f" % (recovered(T.cpu().numpy(), truth), P,
                                                                          fit.mean().item())
        if name.startswith("mvr_fgr, tuple filter on"):
            nt = i32[1].cpu().numpy()
            note += "; tuples per pair %d..%d, status != 0 in %d pairs" % (nt.min(), nt.max(),
                                                                          int((i32[2] != 0).sum().item()))
        notes.append(note)
    ms = [[] for _ in runs]
    for _ in range(a.reps):                      # interleaved: A B C D A B C D ...
        for k, (_, run) in enumerate(runs):
            ms[k].append(event_ms(run))
    med = [sorted(v)[len(v) // 2] for v in ms]
    for k, (name, _) in enumerate(runs):
        print("%-70s median %8.3f ms (min %.3f, max %.3f) = %.3f x mvr_ransac; %s"
              % (name, med[k], min(ms[k]), max(ms[k]), med[k] / med[2], notes[k]), flush=True)


def scene(a):
    from lib.fpfh import correspondences, match_features, register_fgr
    from lib.overlap import FragmentOverlap
    from lib.utils import run_fgr_batch
    import icp_oracle as O
    from synth import synth_scene_fragments
    frags, poses = synth_scene_fragments(n_frag=a.frags)
    fo = FragmentOverlap(frags, "FCGF", 0.025)
    xyz = fo.xyz.cpu().numpy()
    fo.estimate_normals(viewpoints=np.asarray([xyz[fo.off[b]:fo.off[b + 1]].mean(0) for b in range(fo.B)]))
    fo.compute_fpfh(fo.r)
    pairs = np.array([(i, j) for i in range(a.frags) for j in range(i + 1, a.frags)], np.int64)
    register_fgr(fo, pairs[:4])
    torch.cuda.synchronize()

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3
    matches, t_match = clock(lambda: match_features(fo.fpfh, fo.off, pairs))
    (xs, xt), t_gather = clock(lambda: correspondences(fo, pairs, matches))
    counts = np.array([len(m) for m in matches], np.int64)
    _, t_fgr = clock(lambda: run_fgr_batch(xs, xt, counts, device=fo.device))
    print("register_fgr's stages on %d fragments, %d pairs, %d..%d mutual matches (mean %.0f): match_features %.1f ms, "
          "correspondences (Python gather) %.1f ms, run_fgr_batch %.1f ms"
          % (a.frags, len(pairs), counts.min(), counts.max(), counts.mean(), t_match, t_gather, t_fgr), flush=True)
    for tuple_test in (True, False):
        out, dt = clock(lambda: register_fgr(fo, pairs, tuple_test=tuple_test))
        ok = 0
        for k, (i, j) in enumerate(pairs):
            D = np.linalg.inv(O.gt_transform(poses, i, j)) @ out["T"][k]
            c = frags[i].astype(np.float64).mean(0)
            ang = np.rad2deg(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
            ok += ang < 15.0 and np.linalg.norm(D[:3, :3] @ c + D[:3, 3] - c) < 0.3
        print("register_fgr(tuple_test=%s) end to end: %.1f ms; %d of %d pairs within 15 deg / 0.3 m of ground truth; "
              "tuples per pair %d..%d (median %d); status != 0 in %d pairs"
              % (tuple_test, dt, ok, len(pairs), out["n_tuples"].min(), out["n_tuples"].max(),
                 np.median(out["n_tuples"]), int((out["status"] != 0).sum())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=435)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--inliers", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scene", action="store_true")
    ap.add_argument("--frags", type=int, default=30)
    a = ap.parse_args()
    launches(a)
    if a.scene:
        scene(a)


if __name__ == "__main__":
    main()
