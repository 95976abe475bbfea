"""Timing of the information matrices (csrc/info.hip mvr_pair_information) and of the pose-graph refinement
(csrc/posegraph.hip mvr_posegraph_optimize); DESIGN.md 4.22.  HIP events around each call after a warm-up, median over
--reps calls, minimum and maximum stated.

  information   the scene of tools/icp_micro.py: the 30-fragment synthetic scene's 435 pairs on its 0.025 m voxel
                centroids, ground-truth starts perturbed by 2 degrees / sigma 2 cm, max_dist = the index's cell.
                mvr_pair_information and mvr_icp_refine with max_iters = 0 (the same search, seventeen sums instead of
                eleven) alternate call by call, so both see the same clocks
  pose graph    the seeded noisy scenes of tests/posegraph_oracle.py (all pairs; 3 degrees / 5 cm starts) at 30
                fragments / 435 edges and 60 / 1,770, for 1 and 8 scenes: per trial ((6 trials - 2 trials) / 4, both
                tolerances 0) and a run at the default tolerances; beside them mvr_sync_poses (one pass) on the same
                edges, the numpy oracle's whole loop, and LAPACK alone on the oracle's system (numpy cholesky + two
                triangular solves of 6N unknowns, one trial's solve)
  line process  --line_process: mvr_posegraph_optimize_lp (every edge uncertain, mu_scale 0.0025) beside
                mvr_posegraph_optimize on the same scenes, the two alternating call by call, at 2 and at 6 trials:
                the time per trial of each and their ratio
usage: python tools/posegraph_micro.py [--reps 15] [--skip_info] [--skip_graph] [--line_process]"""
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


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def timed(run, reps, warm=3):
    for _ in range(warm):
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
    return ms


def information(reps):
    import icp_oracle as O
    from lib.overlap import FragmentOverlap
    from synth import synth_scene_fragments
    d = torch.device("cuda")
    L = N.lib()
    frags, poses = synth_scene_fragments(n_frag=30)
    fo = FragmentOverlap(frags, "FCGF", 0.025)
    pairs = np.array([(i, j) for i in range(30) for j in range(i + 1, 30)], np.int64)
    rng = np.random.default_rng(0)
    xyz = fo.xyz.cpu().numpy()
    cent = [xyz[fo.off[b]:fo.off[b + 1]] for b in range(fo.B)]
    T0 = np.empty((len(pairs), 4, 4))
    for k, (i, j) in enumerate(pairs):
        T = O.gt_transform(poses, i, j)
        T0[k] = O.perturb(T, (cent[i] @ T[:3, :3].T + T[:3, 3]).mean(0), rng, 2.0, 0.02)
    P = len(pairs)
    gp = torch.from_numpy(pairs).to(d)
    gT = torch.from_numpy(np.ascontiguousarray(T0[:, :3])).to(d)
    T = torch.empty(P, 12, dtype=torch.float64, device=d)
    info = torch.empty(P, 36, dtype=torch.float64, device=d)
    fit, rm, rm2 = (torch.empty(P, dtype=torch.float64, device=d) for _ in range(3))
    nc, nc2, it, st, st2 = (torch.empty(P, dtype=torch.int32, device=d) for _ in range(5))
    head = (N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.off_dev), fo.B, fo.M, fo.r, N.ptr(gp), N.ptr(gT),
            P, fo.r)

    def icp0():
        assert L.mvr_icp_refine(*head, 0, 0.0, 0.0, N.ptr(T), N.ptr(fit), N.ptr(rm), N.ptr(nc), N.ptr(it), N.ptr(st),
                                None, N.stream()) == 0

    def inf():
        assert L.mvr_pair_information(*head, N.ptr(info), N.ptr(nc2), N.ptr(rm2), N.ptr(st2), N.stream()) == 0
    for _ in range(3):
        icp0()
        inf()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):      # alternating: both kernels see the same clocks and the same cache state
        a += timed(icp0, 1, warm=0)
        b += timed(inf, 1, warm=0)
    assert torch.equal(nc, nc2)
    print("%s: %d pairs on %d centroids, cell %.3f m" % (N.source_hash(), P, fo.M, fo.r))
    print("mvr_icp_refine, 0 iterations: median %.3f ms (min %.3f, max %.3f, %d calls)" % (stats(a) + (reps,)))
    print("mvr_pair_information:         median %.3f ms (min %.3f, max %.3f, %d calls); n_corr %d..%d, equal to ICP's"
          % (stats(b) + (reps, int(nc2.min()), int(nc2.max()))), flush=True)


def graph(n, reps, line_process=False):
    import posegraph_oracle as PO
    d = torch.device("cuda")
    L = N.lib()
    scenes = [PO.scene(n, 100 + s, "all", True, 0) for s in range(8)]
    E = len(scenes[0]["ij"])

    def dev(key, dtype=None):
        x = np.stack([s[key] for s in scenes])
        return torch.from_numpy(x.astype(dtype) if dtype else x).to(d).contiguous()
    Rp, tp, ij, info, w, R0, t0 = (dev("R_pair"), dev("t_pair"), dev("ij", np.int32), dev("info"), dev("w"), dev("R0"),
                                  dev("t0"))

    def bench(S, iters, tol_cost, tol_step):
        n_e = torch.full((S,), E, dtype=torch.int32, device=d)
        n_f = torch.full((S,), n, dtype=torch.int32, device=d)
        R = torch.empty(S, n, 9, dtype=torch.float64, device=d)
        t = torch.empty(S, n, 3, dtype=torch.float64, device=d)
        cost = torch.empty(S, 2, dtype=torch.float64, device=d)
        its, status = (torch.empty(S, dtype=torch.int32, device=d) for _ in range(2))
        ws = torch.empty(L.mvr_posegraph_workspace_bytes(S, n, E), dtype=torch.uint8, device=d)

        def run():
            assert L.mvr_posegraph_optimize(N.ptr(Rp), N.ptr(tp), N.ptr(ij), N.ptr(w), N.ptr(info), E, N.ptr(n_e),
                                            N.ptr(n_f), S, n, E, 0, N.ptr(R0), N.ptr(t0), iters, 1e-6, tol_cost,
                                            tol_step, N.ptr(R), N.ptr(t), n, None, N.ptr(cost), N.ptr(its),
                                            N.ptr(status), None, N.ptr(ws), ws.numel(), N.stream()) == 0
        ms = timed(run, reps)
        return stats(ms), its.tolist(), sorted(set(status.tolist())), cost[0].tolist()

    def pair(S, iters):
        """(plain, line process) timings of `iters` trials, alternating call by call"""
        n_e = torch.full((S,), E, dtype=torch.int32, device=d)
        n_f = torch.full((S,), n, dtype=torch.int32, device=d)
        R = torch.empty(S, n, 9, dtype=torch.float64, device=d)
        t = torch.empty(S, n, 3, dtype=torch.float64, device=d)
        cost = torch.empty(S, 2, dtype=torch.float64, device=d)
        line = torch.empty(S, E, dtype=torch.float64, device=d)
        its, status = (torch.empty(S, dtype=torch.int32, device=d) for _ in range(2))
        ws = torch.empty(L.mvr_posegraph_lp_workspace_bytes(S, n, E), dtype=torch.uint8, device=d)

        def plain():
            assert L.mvr_posegraph_optimize(N.ptr(Rp), N.ptr(tp), N.ptr(ij), N.ptr(w), N.ptr(info), E, N.ptr(n_e),
                                            N.ptr(n_f), S, n, E, 0, N.ptr(R0), N.ptr(t0), iters, 1e-6, 0.0, 0.0,
                                            N.ptr(R), N.ptr(t), n, None, N.ptr(cost), N.ptr(its), N.ptr(status), None,
                                            N.ptr(ws), ws.numel(), N.stream()) == 0

        def lp():
            assert L.mvr_posegraph_optimize_lp(N.ptr(Rp), N.ptr(tp), N.ptr(ij), N.ptr(w), N.ptr(info), None, E,
                                               N.ptr(n_e), N.ptr(n_f), S, n, E, 0, N.ptr(R0), N.ptr(t0), iters, 1e-6,
                                               0.0, 0.0, 0.0025, N.ptr(R), N.ptr(t), n, None, N.ptr(cost), N.ptr(its),
                                               N.ptr(status), None, N.ptr(line), None, N.ptr(ws), ws.numel(),
                                               N.stream()) == 0
        for _ in range(3):
            plain()
            lp()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(reps):
            a += timed(plain, 1, warm=0)
            b += timed(lp, 1, warm=0)
        assert its.tolist() == [iters] * S
        return stats(a), stats(b)

    if line_process:
        for S in (1, 8):
            (p2, l2), (p6, l6) = pair(S, 2), pair(S, 6)
            tp_, tl_ = (p6[0] - p2[0]) / 4.0, (l6[0] - l2[0]) / 4.0
            print("line process %d scene%s x %d fragments x %d edges: plain 2 trials %.3f ms (min %.3f, max %.3f), 6 "
                  "trials %.3f ms (min %.3f, max %.3f) -> %.4f ms per trial; line process 2 trials %.3f ms (min %.3f, "
                  "max %.3f), 6 trials %.3f ms (min %.3f, max %.3f) -> %.4f ms per trial; ratio %.4f"
                  % ((S, "s" if S > 1 else "", n, E) + p2 + p6 + (tp_,) + l2 + l6 + (tl_, tl_ / tp_)), flush=True)
        return

    for S in (1, 8):
        (m2, lo2, hi2), _, _, _ = bench(S, 2, 0.0, 0.0)
        (m6, lo6, hi6), _, _, _ = bench(S, 6, 0.0, 0.0)
        (mc, loc, hic), its, st, cost = bench(S, 20, 1e-9, 1e-10)
        print("pose graph %d scene%s x %d fragments x %d edges: 2 trials median %.3f ms (min %.3f, max %.3f), 6 trials "
              "%.3f ms (min %.3f, max %.3f) -> %.3f ms per trial; default tolerances %.3f ms (min %.3f, max %.3f), "
              "trials %s, status %s, cost of scene 0 %.6g -> %.6g"
              % (S, "s" if S > 1 else "", n, E, m2, lo2, hi2, m6, lo6, hi6, (m6 - m2) / 4.0, mc, loc, hic, its, st,
                 cost[0], cost[1]), flush=True)

    # mvr_sync_poses, one pass, on the same edges
    n_e = torch.full((1,), E, dtype=torch.int32, device=d)
    n_f = torch.full((1,), n, dtype=torch.int32, device=d)
    R = torch.empty(1, n, 9, dtype=torch.float64, device=d)
    t = torch.empty(1, n, 3, dtype=torch.float64, device=d)
    status = torch.empty(1, dtype=torch.int32, device=d)
    ws = torch.empty(L.mvr_sync_workspace_bytes(1, n, E), dtype=torch.uint8, device=d)

    def sync():
        assert L.mvr_sync_poses(N.ptr(Rp), N.ptr(tp), N.ptr(ij), N.ptr(w), E, N.ptr(n_e), N.ptr(n_f), 1, n, E, 0, 0,
                                0.1, 0.1, N.ptr(R), N.ptr(t), n, None, None, None, None, N.ptr(status), N.ptr(ws),
                                ws.numel(), N.stream()) == 0
    print("mvr_sync_poses, 1 scene, one pass, the same edges: median %.3f ms (min %.3f, max %.3f)"
          % stats(timed(sync, reps)), flush=True)

    # the host: the oracle's whole loop (numpy, edge by edge), and LAPACK alone on one trial's system
    sc = scenes[0]
    t_or = time.perf_counter()
    out = PO.run(sc)
    t_or = (time.perf_counter() - t_or) * 1e3
    wc, member, _ = PO.edge_weights(n, 0, sc["R_pair"], sc["t_pair"], sc["ij"], sc["w"], sc["info"])
    H, g = PO.system(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], wc, sc["info"], member, 0)
    M = H + 1e-6 * np.diag(np.diag(H))
    host = []
    for _ in range(reps):
        t1 = time.perf_counter()
        C = np.linalg.cholesky(M)
        np.linalg.solve(C.T, np.linalg.solve(C, g))
        host.append((time.perf_counter() - t1) * 1e3)
    print("host: the numpy oracle's loop %.0f ms for %d trials; LAPACK alone (cholesky + two solves, %d unknowns): "
          "median %.3f ms (min %.3f, max %.3f) per trial" % ((t_or, out["iters"], 6 * n) + stats(host)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--skip_info", action="store_true")
    ap.add_argument("--skip_graph", action="store_true")
    ap.add_argument("--line_process", action="store_true",
                    help="pose graph: only mvr_posegraph_optimize_lp beside mvr_posegraph_optimize, alternating")
    a = ap.parse_args()
    if not a.skip_info:
        information(a.reps)
    if not a.skip_graph:
        for n in (30, 60):
            graph(n, a.reps, a.line_process)


if __name__ == "__main__":
    main()
