"""Timing of the batched GPU RANSAC (csrc/ransac.hip mvr_ransac) at the benchmark's --refine / RANSAC
baseline shape: P pairs x 5000 correspondences x 2500 iterations (lib/utils.py:671-709), HIP events, plus
the numpy restatement (oracle/ransac.py) on one pair with fewer iterations, scaled.
--checked: right after it, on the same inputs and in the same process, mvr_ransac_checked (csrc/ransac.hip) at
its defaults (3-point samples, 100000 draws, at most 2500 scored, edge 0.9, distance 0.05) beside mvr_ransac: HIP
events per call after a warm-up, median / min / max over --reps, the ratio, and the split over its four kernels (the
library's own event pairs around each launch, one more run).
usage: python tools/ransac_micro.py [--pairs 435] [--n 5000] [--iters 2500] [--checked]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d_multiview_reg_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lib import _native as N  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=435)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--iters", type=int, default=2500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--checked", action="store_true")
    ap.add_argument("--checked_iters", type=int, default=100000)
    ap.add_argument("--max_validation", type=int, default=2500)
    a = ap.parse_args()
    d = torch.device("cuda")
    g = torch.Generator(device=d).manual_seed(0)
    x1 = torch.rand(a.pairs, a.n, 3, device=d, dtype=torch.float64, generator=g) * 3
    x2 = x1 + 0.01 * torch.randn(a.pairs, a.n, 3, device=d, dtype=torch.float64, generator=g)
    x2[:, a.n // 5:] = torch.rand(a.pairs, a.n - a.n // 5, 3, device=d, dtype=torch.float64, generator=g) * 3
    cnt = torch.full((a.pairs,), a.n, dtype=torch.int32, device=d)
    T = torch.empty(a.pairs, 4, 4, dtype=torch.float64, device=d)
    fit, rmse = (torch.empty(a.pairs, dtype=torch.float64, device=d) for _ in range(2))
    best = torch.empty(a.pairs, dtype=torch.int32, device=d)
    L = N.lib()
    ws = torch.empty(L.mvr_ransac_workspace_bytes(a.pairs, a.iters), dtype=torch.uint8, device=d)

    def run():
        assert L.mvr_ransac(N.ptr(x1), N.ptr(x2), a.n * 3, N.ptr(cnt), a.pairs, 4, a.iters, 0.05, 1, N.ptr(T),
                            N.ptr(fit), N.ptr(rmse), N.ptr(best), None, N.ptr(ws), ws.numel(), N.stream()) == 0
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    flop = 27.0 * a.pairs * a.iters * a.n   # 12 mul + 15 add/sub per (hypothesis, correspondence), fp64
    print("ransac %d pairs x %d corr x %d iters: %.3f ms  %.1f pairs/s  %.1f TF/s fp64 (of 78.6 vector)"
          % (a.pairs, a.n, a.iters, ms, a.pairs / ms * 1e3, flop / ms / 1e9), flush=True)
    print("fitness mean %.3f (inlier fraction 0.2)" % fit.mean().item(), flush=True)
    if a.checked:
        checked(a, L, run, x1, x2, cnt, T, fit, rmse, best)
    from oracle import ransac as O
    h1, h2 = x1[0].cpu().numpy(), x2[0].cpu().numpy()
    it = 40
    t0 = time.time()
    O.ransac(h1, h2, seed=1, iters=it)
    dt = (time.time() - t0) * a.iters / it
    print("numpy restatement (1 thread, vectorised over correspondences): %.2f s per pair (%d iters scaled "
          "from %d) = %.3f pairs/s" % (dt, a.iters, it, 1.0 / dt), flush=True)


def each(run, reps):
    """sorted HIP-event milliseconds of `reps` single calls"""
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)


def checked(a, L, run_plain, x1, x2, cnt, T, fit, rmse, best):
    d = x1.device
    plain_fit = fit.mean().item()
    n_pass, n_valid = (torch.empty(a.pairs, dtype=torch.int32, device=d) for _ in range(2))
    ws = torch.empty(L.mvr_ransac_checked_workspace_bytes(a.pairs, a.checked_iters, a.max_validation),
                     dtype=torch.uint8, device=d)

    def run():
        assert L.mvr_ransac_checked(N.ptr(x1), N.ptr(x2), a.n * 3, N.ptr(cnt), a.pairs, 3, a.checked_iters, 0.05, 1,
                                    a.max_validation, 0.9, 0.05, None, None, -1.0, N.ptr(T), N.ptr(fit), N.ptr(rmse),
                                    N.ptr(best), N.ptr(n_pass), N.ptr(n_valid), None, None, None, N.ptr(ws),
                                    ws.numel(), N.stream()) == 0
    run()
    torch.cuda.synchronize()
    mp, mc = each(run_plain, a.reps), each(run, a.reps)
    med = lambda v: v[len(v) // 2]   # noqa: E731
    print("mvr_ransac (4-point, %d iters):            median %.3f ms (min %.3f, max %.3f)"
          % (a.iters, med(mp), mp[0], mp[-1]), flush=True)
    print("mvr_ransac_checked (3-point, %d draws, cap %d): median %.3f ms (min %.3f, max %.3f) = %.2f x mvr_ransac"
          % (a.checked_iters, a.max_validation, med(mc), mc[0], mc[-1], med(mc) / med(mp)), flush=True)
    npass, nval = n_pass.cpu().numpy(), n_valid.cpu().numpy()
    print("  samples passing the checkers per pair: %d..%d (mean %.0f); scored %d..%d (mean %.0f); fitness mean %.3f "
          "(mvr_ransac: %.3f)" % (npass.min(), npass.max(), npass.mean(), nval.min(), nval.max(), nval.mean(),
                                  fit.mean().item(), plain_fit), flush=True)
    N.prof_set(1)
    run()
    torch.cuda.synchronize()
    split = {k: N.prof_get(i)[0] for k, i in N.RANSAC_CHECKED_PROF.items()}
    N.prof_set(0)
    print("  kernels: " + ", ".join("%s %.3f ms" % kv for kv in split.items()), flush=True)


if __name__ == "__main__":
    main()
