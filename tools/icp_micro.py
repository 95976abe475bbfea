"""Timing of the ICP refinement (csrc/icp.hip mvr_icp_refine, with --method point_to_plane csrc/icp_plane.hip
mvr_icp_refine_plane or with --method generalized csrc/icp_gicp.hip mvr_icp_refine_generalized, both after
csrc/normals.hip mvr_estimate_normals) at the benchmark's scene shape: the 30-fragment synthetic
scene's 435 pairs on its 0.025 m voxel centroids, ground-truth starts perturbed by 2 degrees / sigma 2 cm, max_dist =
the index's cell (0.075 m), both tolerances 0 — 1 and 30 iterations, one pair alone, and for scale the scene's
mvr_radius_overlap_count call on the same index (one 27-cell walk with early exit per query, both directions) and
the host oracle (tests/icp_oracle.py: sklearn kd-tree + numpy SVD) on the first --host_pairs pairs.  HIP events around
each call after a warm-up, median over --reps calls.  point_to_plane and generalized also time the normal estimation
(radius = the cell; generalized takes --epsilon), and every method reports the iterations to convergence at
tolerances 1e-6 from the same starts.  --method colored (csrc/icp_colored.hip mvr_icp_refine_colored)
gives the fragments the colours of tests/colored_icp_oracle.py's field, times csrc/color_grad.hip mvr_color_gradient
beside the normals and runs the point-to-plane calls first, in the same process, so the two methods' figures stand
side by side; with --kernel it goes through its own entry's robust kernels.  --kernel NAME[:K] sends the same calls through csrc/icp_robust.hip
mvr_icp_refine_robust with that robust kernel (l2, huber, cauchy, gm, tukey; K defaults to the voxel size): l2 against
a run without the flag is what the weighted path costs, tukey against l2 what a kernel costs.
A library built with another workgroup size (tools/build_variant.sh icp.hip icp512 -DMVR_ICP_THREADS=512, or
icp_plane.hip plane512 -DMVR_ICP_PLANE_THREADS=512, icp_gicp.hip gicp512 -DMVR_ICP_GICP_THREADS=512, normals.hip
nrm256 -DMVR_NORMALS_THREADS=256, icp_colored.hip col512 -DMVR_ICP_COLORED_THREADS=512, color_grad.hip cg256
-DMVR_COLOR_GRAD_THREADS=256; MVR_LIB=tools/vsp/icp512.so) times that variant.
usage: python tools/icp_micro.py [--method point_to_point|point_to_plane|generalized|colored] [--epsilon 1e-3]
                                 [--lambda_geometric 0.968] [--frags 30] [--reps 7] [--host_pairs 4]
                                 [--kernel tukey:0.025]"""
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
import icp_oracle as O  # noqa: E402
from synth import synth_scene_fragments  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host_pairs", type=int, default=4)
    ap.add_argument("--method", default="point_to_point", choices=["point_to_point", "point_to_plane", "generalized",
                                                                      "colored"])
    ap.add_argument("--epsilon", type=float, default=1e-3)
    ap.add_argument("--lambda_geometric", type=float, default=0.968)
    ap.add_argument("--kernel", default=None, metavar="NAME[:K]")
    a = ap.parse_args()
    d = torch.device("cuda")
    frags, poses = synth_scene_fragments(n_frag=a.frags)
    colored = a.method == "colored"
    if colored:
        import colored_icp_oracle as CO
        world = [np.asarray(f, np.float64) @ poses[b][:3, :3].T + poses[b][:3, 3] for b, f in enumerate(frags)]
        fo = FragmentOverlap(frags, "FCGF", 0.025, colors=[CO.color_field(w) for w in world])
    else:
        fo = FragmentOverlap(frags, "FCGF", 0.025)
    sizes = np.diff(fo.off)
    pairs = np.array([(i, j) for i in range(a.frags) for j in range(i + 1, a.frags)], np.int64)
    rng = np.random.default_rng(0)
    xyz = fo.xyz.cpu().numpy()
    cent = [xyz[fo.off[b]:fo.off[b + 1]] for b in range(fo.B)]
    T0 = np.empty((len(pairs), 4, 4))
    for k, (i, j) in enumerate(pairs):
        T = O.gt_transform(poses, i, j)
        T0[k] = O.perturb(T, (cent[i] @ T[:3, :3].T + T[:3, 3]).mean(0), rng, 2.0, 0.02)
    print("%s: %d fragments of %d..%d centroids (%d in all), %d pairs, cell %.3f m"
          % (N.source_hash(), a.frags, sizes.min(), sizes.max(), fo.M, len(pairs), fo.r), flush=True)
    L = N.lib()
    gp_all = torch.from_numpy(pairs).to(d)
    gT_all = torch.from_numpy(np.ascontiguousarray(T0[:, :3])).to(d)

    def timed(run):
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        return ms

    plane, gicp = a.method == "point_to_plane", a.method == "generalized"
    nrm = None
    if a.kernel is not None:
        from lib.icp import ROBUST_KERNELS
        name, _, k = a.kernel.partition(":")
        kernel, kernel_k = ROBUST_KERNELS.index(name), float(k) if k else 0.025
        print("through mvr_icp_refine_robust: kernel %s, k %g" % (name, kernel_k), flush=True)
    if plane or gicp or colored:
        nrm = torch.empty(fo.M, 3, dtype=torch.float64, device=d)
        nnb = torch.empty(fo.M, dtype=torch.int32, device=d)

        def normals():
            assert L.mvr_estimate_normals(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.off_dev), fo.B,
                                          fo.M, fo.r, fo.r, None, N.ptr(nrm), N.ptr(nnb), N.stream()) == 0
        ms = timed(normals)
        print("mvr_estimate_normals, %d points, radius %.3f: median %.3f ms (min %.3f, max %.3f); neighbours %d..%d"
              % (fo.M, fo.r, ms[len(ms) // 2], ms[0], ms[-1], int(nnb.min()), int(nnb.max())), flush=True)
    if colored:
        inten = torch.empty(fo.M, dtype=torch.float64, device=d)
        grad = torch.empty(fo.M, 3, dtype=torch.float64, device=d)

        def gradients():
            assert L.mvr_color_gradient(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(nrm), N.ptr(fo.colors),
                                        N.ptr(fo.off_dev), fo.B, fo.M, fo.r, fo.r, N.ptr(inten), N.ptr(grad),
                                        N.ptr(nnb), N.stream()) == 0
        ms = timed(gradients)
        print("mvr_color_gradient, %d points, radius %.3f: median %.3f ms (min %.3f, max %.3f); largest gradient %.3g"
              % (fo.M, fo.r, ms[len(ms) // 2], ms[0], ms[-1], float(grad.abs().max())), flush=True)

    def bench(rows, iters, what, tol=0.0, method=a.method):
        plane, gicp, colored = method == "point_to_plane", method == "generalized", method == "colored"
        P = len(rows)
        gp, gT = gp_all[rows].contiguous(), gT_all[rows].contiguous()
        T = torch.empty(P, 12, dtype=torch.float64, device=d)
        fit, rm = (torch.empty(P, dtype=torch.float64, device=d) for _ in range(2))
        nc, it, st = (torch.empty(P, dtype=torch.int32, device=d) for _ in range(3))

        tail = (fo.r, N.ptr(gp), N.ptr(gT), P, fo.r, iters, tol, tol, N.ptr(T), N.ptr(fit), N.ptr(rm), N.ptr(nc),
                N.ptr(it), N.ptr(st), None, N.stream())

        def run():
            if colored:
                assert L.mvr_icp_refine_colored(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(nrm),
                                                N.ptr(inten), N.ptr(grad), N.ptr(fo.off_dev), fo.B, fo.M, *tail[:5],
                                                a.lambda_geometric, kernel if a.kernel is not None else 0,
                                                kernel_k if a.kernel is not None else 0.0, *tail[5:-1], None,
                                                tail[-1]) == 0
            elif a.kernel is not None:
                assert L.mvr_icp_refine_robust(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(nrm),
                                               N.ptr(fo.off_dev), fo.B, fo.M, *tail[:4],
                                               ["point_to_point", "point_to_plane", "generalized"].index(method),
                                               tail[4], a.epsilon, kernel, kernel_k, *tail[5:-1], None,
                                               tail[-1]) == 0
            elif gicp:
                assert L.mvr_icp_refine_generalized(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(nrm),
                                                    N.ptr(fo.off_dev), fo.B, fo.M, *tail[:5], a.epsilon,
                                                    *tail[5:]) == 0
            elif plane:
                assert L.mvr_icp_refine_plane(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(nrm),
                                              N.ptr(fo.off_dev), fo.B, fo.M, *tail) == 0
            else:
                assert L.mvr_icp_refine(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.off_dev), fo.B,
                                        fo.M, *tail) == 0
        ms = timed(run)
        if tol > 0.0:
            its = it.cpu().numpy()
            print("%s %s, tolerances %g, cap %d: median %.3f ms (min %.3f, max %.3f); iterations min %d, median %d, "
                  "mean %.1f, max %d; %d of %d at the cap; rmse mean %.4f"
                  % (method, what, tol, iters, ms[len(ms) // 2], ms[0], ms[-1], its.min(), int(np.median(its)),
                     its.mean(), its.max(), int((st.cpu().numpy() & 2 != 0).sum()), P, float(rm.mean())), flush=True)
            return ms[len(ms) // 2]
        print("%s %s, %d iterations: median %.3f ms (min %.3f, max %.3f, %d calls); fitness %.3f..%.3f, rmse mean "
              "%.4f, status %s" % (method, what, iters, ms[len(ms) // 2], ms[0], ms[-1], a.reps, float(fit.min()),
                                   float(fit.max()), float(rm.mean()), sorted(set(st.tolist()))), flush=True)
        return ms[len(ms) // 2]

    every = torch.arange(len(pairs), device=d)
    if colored:      # point-to-plane first, in the same process: the figures the coloured ones stand beside
        p1 = bench(every, 1, "%d pairs" % len(pairs), method="point_to_plane")
        p30 = bench(every, 30, "%d pairs" % len(pairs), method="point_to_plane")
        print("point_to_plane per evaluation: %.3f ms over the scene" % ((p30 - p1) / 29.0), flush=True)
    t0 = bench(every, 0, "%d pairs" % len(pairs))
    t1 = bench(every, 1, "%d pairs" % len(pairs))
    t30 = bench(every, 30, "%d pairs" % len(pairs))
    one = bench(every[:1], 30, "pair (0, 1) alone")
    bench(every, 30, "%d pairs" % len(pairs), tol=1e-6)
    print("per evaluation: %.3f ms over the scene ((30 - 1 iterations) / 29), %.3f ms for the pair alone"
          % ((t30 - t1) / 29.0, one / 31.0), flush=True)

    # the overlap gate on the same index and transforms: both directions of every pair, early exit at the first hit
    Tg = np.empty((len(pairs), 2, 3, 4))
    Tg[:, 0], Tg[:, 1] = T0[:, :3], np.linalg.inv(T0)[:, :3]
    gTg = torch.from_numpy(Tg).to(d)
    cnt = torch.empty(len(pairs), 2, dtype=torch.int32, device=d)

    def gate():
        assert L.mvr_radius_overlap_count(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.off_dev), fo.B,
                                          fo.M, N.ptr(gp_all), N.ptr(gTg), len(pairs), fo.max_points, fo.r,
                                          N.ptr(cnt), N.stream()) == 0
    ms = timed(gate)
    print("mvr_radius_overlap_count, %d pairs x 2 directions: median %.3f ms (min %.3f, max %.3f); the evaluation "
          "alone (0 iterations) %.3f ms" % (len(pairs), ms[len(ms) // 2], ms[0], ms[-1], t0), flush=True)

    host = []
    for k in range(0 if plane or gicp or colored else min(a.host_pairs, len(pairs))):
        i, j = pairs[k]
        t = time.perf_counter()
        r = O.icp(cent[i], cent[j], T0[k], fo.r, 30, 0.0, 0.0)
        host.append((time.perf_counter() - t) * 1e3)
        assert r["iters"] == 30
    host.sort()
    if host:
        print("host oracle (kd-tree + SVD), 30 iterations: median %.1f ms per pair over %d pairs -> about %.0f ms for "
              "%d pairs one after the other (extrapolated); the GPU's pair alone %.3f ms"
              % (host[len(host) // 2], len(host), host[len(host) // 2] * len(pairs), len(pairs), one), flush=True)


if __name__ == "__main__":
    main()
