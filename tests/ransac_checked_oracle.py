"""RANSAC with correspondence checkers restated in numpy (TEST ORACLE for csrc/ransac.hip mvr_ransac_checked;
the semantics are in include/mvreg.h).  The draws, the Umeyama fit, the evaluation and the selection are
oracle/ransac.py's (draws and fits vectorised over the iterations here and pinned to O.draws / O.umeyama by
tests/test_ransac_checked_host.py).

Iteration `it` passes when, in this order: (1) edge_sim > 0: no correspondence drawn twice; (2) edge_sim > 0: every
pair j < k of the draws has ls2 >= sim2 * lt2 and lt2 >= sim2 * ls2 on the squared lengths; (3) the fit;
(4) check_dist > 0: every sample point within check_dist of its match under the fit; (5) normals given: every
rotated source normal within the cone of its target normal.  The first max_validation passing iterations are
scored over all correspondences (O.evaluate) and the best is picked (O.select).

`undecided[it]`: a comparison of that iteration is too close to call between two correct implementations — an edge
comparison with |lhs - rhs| <= 1e-9 max(lhs, rhs), or a distance / normal value within 1e-7 (relative / absolute) of
its threshold (the GPU's Jacobi fit and LAPACK's differ by about 1e-9) — and no other comparison rejects it.
"""
import numpy as np

from oracle import ransac as O

EDGE_TOL, FIT_TOL = 1e-9, 1e-7


# ------------------------------------------------------------------------------------------------ shared test inputs
# (tests/test_ransac_checked_host.py caps the undecided share on exactly what tests/test_gpu_ransac_checked.py runs)
SEED = 11
MAX_DIST = 0.05
PARITY_N, PARITY_ITERS, PARITY_CAP = (3, 37, 300, 1000), (100, 1000, 4097), 200
MODES = {"edge": (0.9, 0.0), "dist": (0.0, MAX_DIST), "both": (0.9, MAX_DIST)}   # (edge_sim, check_dist)
QUALITY = dict(n=2000, inl=0.05, data_seed=21, seed=0, iters=100000, max_validation=2500, edge_sim=0.9)
NORMAL_DEG = 20.0


def corr(n, inl, seed, noise=0.005, normals=False):
    """tests/test_gpu_ransac.py's _corr: n correspondences of a random motion, a share `inl` of them inliers with
    `noise`, the rest uniform.  normals: also unit normals, the inliers' rotated by the motion, the outliers' random."""
    from synth import random_rotation
    rng = np.random.default_rng(seed)
    R, t = random_rotation(rng), rng.normal(0, 1.0, 3)
    x1 = rng.uniform(-1.5, 1.5, (n, 3))
    x2 = x1 @ R.T + t + np.clip(rng.normal(0, noise, (n, 3)), -0.025, 0.025)
    out = rng.permutation(n)[int(round(n * inl)):]
    x2[out] = rng.uniform(-1.5, 1.5, (len(out), 3)) + t
    if not normals:
        return x1, x2, R, t
    n1 = rng.normal(0, 1, (n, 3))
    n1 /= np.linalg.norm(n1, axis=1, keepdims=True)
    n2 = n1 @ R.T
    rnd = rng.normal(0, 1, (len(out), 3))
    n2[out] = rnd / np.linalg.norm(rnd, axis=1, keepdims=True)
    return x1, x2, R, t, n1, n2


def parity_inputs(n, normals=False):
    """three pairs of n rows with inlier shares 0.05, 0.3, 0.8 and ragged counts [n, n - 5, n // 2]"""
    data = [corr(n, f, seed=10 + p, normals=normals) for p, f in enumerate((0.05, 0.3, 0.8))]
    arrays = [np.stack([d[i] for d in data]) for i in ((0, 1, 4, 5) if normals else (0, 1))]
    return arrays, [n, max(n - 5, 0), n // 2]


def draws_all(seed, p, iters, k, n):
    """[iters, k] int64: O.draws(seed, p, it, k, n) for every it"""
    it = np.arange(iters, dtype=np.uint64)[:, None]
    j = np.arange(k, dtype=np.uint64)[None, :]
    ctr = (np.uint64(p) << np.uint64(40)) | (it << np.uint64(8)) | j
    with np.errstate(over="ignore"):
        z = np.uint64(seed & O.M64) + ctr * np.uint64(O.GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % np.uint64(n)).astype(np.int64)


def umeyama_all(src, dst):
    """O.umeyama on [m, k, 3] samples at once: R [m,3,3], t [m,3] (the same sequential sums)"""
    m, k = src.shape[0], src.shape[1]
    if m == 0:
        return np.zeros((0, 3, 3)), np.zeros((0, 3))
    ms = np.zeros((m, 3))
    md = np.zeros((m, 3))
    for j in range(k):
        ms = ms + src[:, j]
        md = md + dst[:, j]
    ms = ms / k
    md = md / k
    H = np.zeros((m, 3, 3))
    for r in range(3):
        for c in range(3):
            acc = np.zeros(m)
            for j in range(k):
                acc = acc + (dst[:, j, r] - md[:, r]) * (src[:, j, c] - ms[:, c])
            H[:, r, c] = acc / k
    U, _, Vt = np.linalg.svd(H)
    sg = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
    D = np.tile(np.eye(3), (m, 1, 1))
    D[:, 2, 2] = sg
    R = U @ D @ Vt
    t = md - np.einsum("mij,mj->mi", R, ms)
    return R, t


def _rot(R, v):
    """rows e of R v: (R_e0 v_0 + R_e1 v_1) + R_e2 v_2 for R [m,3,3], v [m,3] -> [m,3]"""
    return np.stack([(R[:, e, 0] * v[:, 0] + R[:, e, 1] * v[:, 1]) + R[:, e, 2] * v[:, 2] for e in range(3)], 1)


def ransac_checked(x1, x2, seed=0, ransac_n=3, max_dist=0.05, iters=100000, max_validation=2500, edge_sim=0.9,
                   check_dist=None, n1=None, n2=None, normal_cos=-1.0, p=0, hyps=None, valid=None):
    """One pair -> dict: bits, undecided (bool [iters]), n_pass, n_valid, valid (int [n_valid], the oracle's own
    list), own [n_valid, 12] (the oracle's fits of its list), and the selection T, fitness, rmse, best_iter, cnt,
    err.  `valid` + `hyps` [len(valid), 12] (the GPU's list and its exported hypotheses) replace the oracle's own
    list and fits in the evaluation, as O.ransac(hyps=...) does."""
    x1 = np.asarray(x1, np.float64)
    x2 = np.asarray(x2, np.float64)
    n, k = x1.shape[0], ransac_n
    check_dist = max_dist if check_dist is None else check_dist
    normals = n1 is not None and n2 is not None
    out = {"bits": np.zeros(iters, bool), "undecided": np.zeros(iters, bool), "n_pass": 0, "n_valid": 0,
           "valid": np.zeros(0, np.int64), "own": np.zeros((0, 12)), "T": np.eye(4), "fitness": 0.0, "rmse": 0.0,
           "best_iter": -1, "cnt": np.zeros(0, np.int64), "err": np.zeros(0)}
    if n < k:
        return out
    idx = draws_all(seed, p, iters, k, n)
    alive = np.ones(iters, bool)       # not rejected so far
    close = np.zeros(iters, bool)      # some comparison too close to call
    if edge_sim > 0:
        srt = np.sort(idx, 1)
        alive &= ~(srt[:, 1:] == srt[:, :-1]).any(1)
        sim2 = edge_sim * edge_sim
        s, d = x1[idx], x2[idx]
        for j in range(k):
            for l in range(j + 1, k):
                a, b = s[:, j] - s[:, l], d[:, j] - d[:, l]
                ls2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
                lt2 = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
                for lhs, rhs in ((ls2, sim2 * lt2), (lt2, sim2 * ls2)):
                    near = np.abs(lhs - rhs) <= EDGE_TOL * np.maximum(lhs, rhs)
                    alive &= (lhs >= rhs) | near
                    close |= near
    if check_dist > 0 or normals:
        sel = np.flatnonzero(alive)
        R, t = umeyama_all(x1[idx[sel]], x2[idx[sel]])
        ok = np.ones(len(sel), bool)
        near_any = np.zeros(len(sel), bool)
        for j in range(k):
            c = idx[sel, j]
            if check_dist > 0:
                cd2 = check_dist * check_dist
                df = (_rot(R, x1[c]) + t) - x2[c]
                dd = ((0.0 + df[:, 0] * df[:, 0]) + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]
                near = np.abs(dd - cd2) <= FIT_TOL * cd2
                ok &= (dd < cd2) | near
                near_any |= near
            if normals:
                r = _rot(R, n1[c])
                dot = (r[:, 0] * n2[c, 0] + r[:, 1] * n2[c, 1]) + r[:, 2] * n2[c, 2]
                near = np.abs(dot - normal_cos) <= FIT_TOL
                ok &= (dot >= normal_cos) | near
                near_any |= near
        alive[sel[~ok]] = False
        close[sel[near_any]] = True
    out["undecided"] = alive & close
    # an undecided iteration counts as passing in the oracle's own list: the tests compare lists only where no
    # undecided iteration precedes the cap
    out["bits"] = alive
    mine = np.flatnonzero(alive)
    out["n_pass"] = len(mine)
    mine = mine[:max_validation]
    out["n_valid"] = len(mine)
    out["valid"] = mine
    R, t = umeyama_all(x1[idx[mine]], x2[idx[mine]])
    out["own"] = np.concatenate([R.reshape(-1, 9), t], 1)
    use_list = mine if valid is None else np.asarray(valid, np.int64)
    use_hyp = out["own"] if hyps is None else np.asarray(hyps, np.float64)
    assert len(use_hyp) == len(use_list)
    cnt = np.zeros(len(use_list), np.int64)
    err = np.zeros(len(use_list))
    for i in range(len(use_list)):
        cnt[i], err[i] = O.evaluate(x1, x2, use_hyp[i, :9].reshape(3, 3), use_hyp[i, 9:], max_dist)
    b, fit, rmse = O.select(cnt, err, n)
    out.update(cnt=cnt, err=err, fitness=fit, rmse=rmse)
    if b >= 0:
        out["best_iter"] = int(use_list[b])
        out["T"][:3, :3] = use_hyp[b, :9].reshape(3, 3)
        out["T"][:3, 3] = use_hyp[b, 9:]
    return out
