"""Fast Global Registration over given correspondences restated in numpy (TEST ORACLE for csrc/fgr.hip mvr_fgr; the
semantics are in include/mvreg.h, the maths in DESIGN.md 4.28).  Zhou, Park, Koltun, ECCV 2016, from the maths: no
line of Open3D's FastGlobalRegistration is followed.  The draws are oracle/ransac.py's (vectorised by
ransac_checked_oracle.draws_all), the final scoring is oracle.ransac.evaluate.

Steps (one pair): A the tuple filter, B the normalisation, C the graduated non-convexity, D the output; `fgr` returns
what the kernel returns plus what tests/test_fgr_host.py pins (the margins of the tuple comparisons, the test at
which the cap was reached, the final distances).  H and g are accumulated in full (27 products of J) where the kernel
sums the 16 moments H is made of: the two differ by rounding only.
"""
import functools

import numpy as np

from oracle import ransac as O
from ransac_checked_oracle import corr, draws_all

# ------------------------------------------------------------------------------------------------ shared test inputs
CASES = [(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0), (4, 1.0), (37, 0.8), (63, 0.5), (64, 0.5), (65, 0.5),
         (300, 0.3), (1025, 0.5), (2000, 0.05)]     # (n, inlier share)
ROWS, DATA_SEED, SEED, MAX_DIST = 2000, 40, 0, 0.05
DEFAULTS = dict(max_dist=MAX_DIST, iters=64, division_factor=1.4, tuple_scale=0.95, max_tuples=1000, tuple_factor=100)


def case(p):
    """pair p of the batch: (x1 [n,3], x2 [n,3], R, t) with x2 ~ R x1 + t on the inliers"""
    n, inl = CASES[p]
    if n == 0:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.eye(3), np.zeros(3)
    return corr(n, inl, seed=DATA_SEED + p)


@functools.lru_cache(maxsize=None)
def batch():
    """(x1 [12,2000,3], x2, counts [12]): every case padded with zero rows"""
    x1 = np.zeros((len(CASES), ROWS, 3))
    x2 = np.zeros((len(CASES), ROWS, 3))
    for p, (n, _) in enumerate(CASES):
        a, b, _, _ = case(p)
        x1[p, :n], x2[p, :n] = a, b
    for a in (x1, x2):
        a.setflags(write=False)
    return x1, x2, np.array([n for n, _ in CASES], np.int32)


@functools.lru_cache(maxsize=None)
def batch_results(tuple_test):
    """the oracle on every case of the batch (seed 0, max_dist 0.05, the defaults): a list of fgr()'s dicts"""
    x1, x2, counts = batch()
    return [fgr(x1[p, :counts[p]], x2[p, :counts[p]], seed=SEED, p=p, tuple_test=tuple_test)
            for p in range(len(CASES))]


def stacked(results, iters=64):
    """a list of fgr() dicts -> the arrays lib.utils.run_fgr_batch returns"""
    out = {k: np.stack([np.asarray(r[k]) for r in results]) for k in ("T", "fitness", "rmse", "trace")}
    for k in ("n_used", "n_tuples", "status"):
        out[k] = np.array([r[k] for r in results], np.int32)
    return out


def pose_error(T, R, t, at=None):
    """(degrees between T's rotation and R, metres between T x and R x + t at the point `at`, default the origin)"""
    at = np.zeros(3) if at is None else np.asarray(at, np.float64)
    c = np.clip((np.trace(T[:3, :3].T @ R) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.rad2deg(np.arccos(c))), float(np.linalg.norm((T[:3, :3] @ at + T[:3, 3]) - (R @ at + t)))


# ---------------------------------------------------------------------------------------------------------- the steps
def tuple_filter(x1, x2, seed, p, tuple_factor, max_tuples, tuple_scale):
    """step A -> (used rows int64 [3 n_tuples] in draw order, n_tuples, the smallest relative gap |lhs - rhs| /
    max(lhs, rhs) over every comparison between distinct draws (inf: none), the test that filled the cap or -1)"""
    n = len(x1)
    idx = draws_all(seed, p, tuple_factor * n, 3, n)
    ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    distinct = ok.copy()
    s2 = tuple_scale * tuple_scale
    gap = np.inf
    s, d = x1[idx], x2[idx]
    for j, l in ((0, 1), (0, 2), (1, 2)):
        a, b = s[:, j] - s[:, l], d[:, j] - d[:, l]
        ls2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        lt2 = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
        for lhs, rhs in ((ls2, s2 * lt2), (lt2, s2 * ls2)):
            ok &= lhs >= rhs
            if distinct.any():
                rel = np.abs(lhs - rhs)[distinct] / np.maximum(lhs, rhs)[distinct]
                gap = min(gap, float(rel.min()))
    passing = np.flatnonzero(ok)
    kept = passing[:max_tuples]
    full_at = int(passing[max_tuples - 1]) if len(passing) >= max_tuples else -1
    return idx[kept].reshape(-1), len(kept), gap, full_at


def solve6(H, g):
    """icp_core.hpp solve6: xi = -H^-1 g by Cholesky; None when a pivot is not above 1e-12 of the largest diagonal"""
    L = np.zeros((6, 6))
    floor_ = 1e-12 * max(0.0, float(np.max(np.diag(H))))
    for j in range(6):
        d = H[j, j] - float(L[j, :j] @ L[j, :j])
        if not d > floor_:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - float(L[i, :i] @ y[:i])) / L[i, i]
    xi = np.zeros(6)
    for i in range(5, -1, -1):
        xi[i] = (y[i] - float(L[i + 1:, i] @ xi[i + 1:])) / L[i, i]
    return xi


def euler(xi):
    """Rz(xi2) Ry(xi1) Rx(xi0) (icp_core.hpp SixDofModel::solve)"""
    cx, sx, cy, sy, cz, sz = np.cos(xi[0]), np.sin(xi[0]), np.cos(xi[1]), np.sin(xi[1]), np.cos(xi[2]), np.sin(xi[2])
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]])


def _failed(status, iters):
    return {"T": np.eye(4), "fitness": 0.0, "rmse": 0.0, "n_used": 0, "n_tuples": 0, "status": status,
            "trace": np.full((iters, 2), -1.0), "gap": np.inf, "full_at": -1, "dist": np.zeros(0)}


def fgr(x1, x2, seed=0, p=0, max_dist=MAX_DIST, iters=64, division_factor=1.4, tuple_test=True, tuple_scale=0.95,
        max_tuples=1000, tuple_factor=100):
    """One pair -> dict: T [4,4], fitness, rmse, n_used, n_tuples, status, trace [iters,2] (mvr_fgr's outputs), and
    gap, full_at (tuple_filter's), dist [n] (the final distances |T x1 - x2|)."""
    x1 = np.asarray(x1, np.float64).reshape(-1, 3)
    x2 = np.asarray(x2, np.float64).reshape(-1, 3)
    n = len(x1)
    if not (np.isfinite(x1).all() and np.isfinite(x2).all()):
        return _failed(4, iters)
    if n < 3:
        return _failed(1, iters)
    # B (before A, as the kernel: A's rows are stored normalised)
    mu1, mu2 = x1.sum(0) / n, x2.sum(0) / n
    scale = np.sqrt(max(((x1 - mu1) ** 2).sum(1).max(), ((x2 - mu2) ** 2).sum(1).max()))
    if not scale > 0.0:
        return _failed(1, iters)
    gap, full_at, n_tuples = np.inf, -1, 0
    if tuple_test:
        used, n_tuples, gap, full_at = tuple_filter(x1, x2, seed, p, tuple_factor, max_tuples, tuple_scale)
        if len(used) < 3:
            out = _failed(1, iters)
            out["gap"] = gap
            return out
    else:
        used = np.arange(n)
    P, Q = (x1[used] - mu1) / scale, (x2[used] - mu2) / scale
    m = len(used)
    delta = max_dist / scale
    # C
    R, t, mu, status = np.eye(3), np.zeros(3), 1.0, 0
    trace = np.full((iters, 2), -1.0)
    for k in range(iters):
        if k % 4 == 0 and mu > delta * delta:
            mu = mu / division_factor
        Pm = P @ R.T + t
        e = Pm - Q
        e2 = (e * e).sum(1)
        w = (mu / (e2 + mu)) ** 2
        trace[k] = mu, float((w * e2).sum() / m)
        J = np.zeros((m, 3, 6))      # row r of J: d e_r / d (omega, v) = [-[p']x | I]
        J[:, 0, 1], J[:, 0, 2] = Pm[:, 2], -Pm[:, 1]
        J[:, 1, 0], J[:, 1, 2] = -Pm[:, 2], Pm[:, 0]
        J[:, 2, 0], J[:, 2, 1] = Pm[:, 1], -Pm[:, 0]
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
        H = np.einsum("m,mra,mrb->ab", w, J, J)
        g = np.einsum("m,mra,mr->a", w, J, e)
        xi = solve6(H, g)
        if xi is None:
            status |= 8
            break
        D = euler(xi)
        R, t = D @ R, D @ t + xi[3:]
    # D
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = scale * t + mu2 - R @ mu1
    good, err = O.evaluate(x1, x2, T[:3, :3], T[:3, 3], max_dist)
    dist = np.linalg.norm(x1 @ T[:3, :3].T + T[:3, 3] - x2, axis=1)
    return {"T": T, "fitness": good / n, "rmse": float(np.sqrt(err / good)) if good else 0.0, "n_used": m,
            "n_tuples": n_tuples, "status": status, "trace": trace, "gap": gap, "full_at": full_at, "dist": dist}
