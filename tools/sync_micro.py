"""Timing of the pose synchronisation (csrc/sync.hip mvr_sync_poses) at the benchmark's scene shape: 30 fragments,
435 pairs (30 % of them outliers) — 0 IRLS passes, 5 passes, and S = 8 such scenes in one launch; HIP events around
each call, median over --reps calls.  Plus the numpy oracle's eigh + solve on the host for the same scene.
--stamps: with a library built with -DMVR_SYNC_STAMPS (tools/build_variant.sh sync.hip sync_stamps -DMVR_SYNC_STAMPS,
MVR_LIB=tools/vsp/sync_stamps.so), where the first pass of one scene spends its time, phase by phase.
usage: python tools/sync_micro.py [--frags 30] [--reps 30] [--stamps]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d_multiview_reg_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lib import _native as N  # noqa: E402
import sync_oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=30)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--stamps", action="store_true")
    a = ap.parse_args()
    d = torch.device("cuda")
    n = a.frags
    scenes = [O.make_scene(n, O.complete_edges(n), 100 + s, 0.01, 0.01, 0.3) for s in range(8)]
    E = len(scenes[0]["ij"])
    Rp = torch.from_numpy(np.stack([s["R_pair"] for s in scenes])).to(d)
    tp = torch.from_numpy(np.stack([s["t_pair"] for s in scenes])).to(d)
    ij = torch.from_numpy(np.stack([s["ij"] for s in scenes]).astype(np.int32)).to(d)
    L = N.lib()

    def bench(S, irls):
        n_e = torch.full((S,), E, dtype=torch.int32, device=d)
        n_f = torch.full((S,), n, dtype=torch.int32, device=d)
        R = torch.empty(S, n, 9, dtype=torch.float64, device=d)
        t = torch.empty(S, n, 3, dtype=torch.float64, device=d)
        status = torch.empty(S, dtype=torch.int32, device=d)
        ws = torch.empty(L.mvr_sync_workspace_bytes(S, n, E), dtype=torch.uint8, device=d)

        def run():
            assert L.mvr_sync_poses(N.ptr(Rp), N.ptr(tp), N.ptr(ij), None, E, N.ptr(n_e), N.ptr(n_f), S, n, E, 0, irls,
                                    0.1, 0.1, N.ptr(R), N.ptr(t), n, None, None, None, None, N.ptr(status), N.ptr(ws),
                                    ws.numel(), N.stream()) == 0
        for _ in range(3):
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
        if a.stamps and S == 1:   # the kernel's 100 MHz stamps of scene 0, pass 0, in the workspace's spare bytes
            st = ws[-256:].view(torch.int64).cpu().numpy()
            names = ["build L", "invert L", "subspace iteration (%d steps)" % st[31], "rotations + build A",
                     "invert A", "translations", "residuals + weights"]
            print("  pass 0 of %d: " % (irls + 1) + ", ".join("%s %.1f us" % (nm, (st[k + 1] - st[k]) / 100.0)
                                                            for k, nm in enumerate(names)), flush=True)
        # back to back for about half a second: one short call on an idle device also measures its clock ramp
        k = max(20, int(500.0 / ms[len(ms) // 2]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            run()
        e1.record()
        torch.cuda.synchronize()
        print("sync %d scene%s x %d fragments x %d edges, %d IRLS passes: median %.3f ms (min %.3f, max %.3f, "
              "%d calls), %.3f ms per call over %d calls back to back, status %s"
              % (S, "s" if S > 1 else "", n, E, irls, ms[len(ms) // 2], ms[0], ms[-1], a.reps,
                 e0.elapsed_time(e1) / k, k, sorted(set(status.tolist()))), flush=True)
        return ms[len(ms) // 2]

    one0 = bench(1, 0)
    bench(1, 5)
    bench(8, 0)
    bench(8, 5)
    sc = scenes[0]
    member = np.ones(n, bool)
    Lm = O.rotation_laplacian(sc["R_pair"], sc["ij"], sc["w"], member)
    A = np.random.default_rng(0).standard_normal((n - 1, n - 1))
    A = A @ A.T + n * np.eye(n - 1)
    b = np.ones((n - 1, 3))
    host = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        np.linalg.eigh(Lm)
        np.linalg.solve(A, b)
        host.append((time.perf_counter() - t0) * 1e3)
    host.sort()
    print("host LAPACK (numpy eigh %d x %d + solve %d x %d, one pass): median %.3f ms"
          % (3 * n, 3 * n, n - 1, n - 1, host[len(host) // 2]), flush=True)
    print("single scene, 0 passes: %.2f %% of a 39.85 ms step" % (100.0 * one0 / 39.85), flush=True)


if __name__ == "__main__":
    main()
