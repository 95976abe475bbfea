"""numpy restatement of the robust kernels on the three ICP loops (csrc/icp_robust.hip mvr_icp_refine_robust), on top
of icp_oracle.evaluate, icp_plane_oracle's Cholesky and increment and gicp_oracle's skew, and its own test case.

Open3D is absent, so parity is pinned to the semantics stated here (include/mvreg.h) and to ground
truth.  The loops are those of icp_oracle.icp, icp_plane_oracle.icp_plane and gicp_oracle.gicp; what differs is that
every valid correspondence enters the solve with the weight w(r) of its residual at the T the solve starts from:

    kernel    w(r), k > 0                                method            r
    l2        1                                          point_to_point    |q - y|
    huber     k / max(|r|, k)                            point_to_plane    (q - y) . n
    cauchy    1 / (1 + (r / k)^2)                        generalized       sqrt(d^T A d), d = q - y, A = M^-1
    gm        k / (k + r^2)^2
    tukey     (1 - (r / k)^2)^2 for |r| <= k, else 0

    point_to_point:   weighted Kabsch on the original source points; not sum w > 0: status |= 8; break (T kept)
    point_to_plane:   H = sum w a a^T, g = sum w a b; generalized: H = sum w G^T A G, g = sum w G^T A d; a failed
                      pivot (all weights zero: the first): status |= 8; break (T kept)
    eval(T), fitness, rmse, n_corr, the least counts (3 / 6 / 6, unweighted), the stopping rule and the other status
    bits are the plain loops'.  w_sum = sum w over the valid correspondences of the returned T's evaluation.

Besides the margins of the plain oracles every solve reports its condition: cond(H) of the 6 x 6 system, and for
point-to-point s0 / s1 of the weighted covariance's singular values (the rotation is determined to about eps s0 / s1;
a target of one point, or every weight on one correspondence, leaves it undetermined: inf).
"""
import numpy as np

import gicp_oracle as GO
import icp_oracle as O
import icp_plane_oracle as PO

KERNELS = ("l2", "huber", "cauchy", "gm", "tukey")
METHODS = ("point_to_point", "point_to_plane", "generalized")
MIN_CORR = {"point_to_point": 3, "point_to_plane": 6, "generalized": 6}


def weight(kernel, k, r):
    """w(r) per element; k is not looked at for 'l2'"""
    r = np.asarray(r, np.float64)
    if kernel == "l2":
        return np.ones_like(r)
    if kernel == "huber":
        return k / np.maximum(np.abs(r), k)
    if kernel == "cauchy":
        return 1.0 / (1.0 + (r / k) ** 2)
    if kernel == "gm":
        return k / (k + r * r) ** 2
    if kernel == "tukey":
        return np.where(np.abs(r) <= k, (1.0 - (r / k) ** 2) ** 2, 0.0)
    raise ValueError(kernel)


def weighted_kabsch(x, y, w):
    """argmin_{R, t} sum w_i |R x_i + t - y_i|^2, R in SO(3) -> 3x4; None unless sum w > 0"""
    W = w.sum()
    if not W > 0:
        return None
    mx, my = (w[:, None] * x).sum(0) / W, (w[:, None] * y).sum(0) / W
    U, _, Vt = np.linalg.svd((w[:, None] * (x - mx)).T @ (y - my))
    R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    return np.concatenate([R, (my - R @ mx)[:, None]], 1)


def kabsch_cond(x, y, w):
    """s0 / s1 of the weighted, centred covariance (inf for s1 == 0)"""
    W = w.sum()
    mx, my = (w[:, None] * x).sum(0) / W, (w[:, None] * y).sum(0) / W
    sv = np.linalg.svd((w[:, None] * (x - mx)).T @ (y - my), compute_uv=False)
    return float(sv[0] / sv[1]) if sv[1] > 0 else np.inf


def residuals(method, src, tgt, src_normals, tgt_normals, T, max_dist, epsilon=GO.EPSILON):
    """the residuals r of eval(T)'s valid correspondences, in source order"""
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64)[:3]
    st = O.evaluate(src, tgt, T, max_dist)
    if st["n_corr"] == 0:
        return np.zeros(0)
    return _terms(method, src, tgt, src_normals, tgt_normals, T, st, tgt[0], epsilon)[0]


def _terms(method, src, tgt, ns, nt, T, st, c, epsilon):
    """the valid correspondences of state st at T -> (residuals [k], what the solve needs)"""
    v = st["valid"]
    x, y = src[v], tgt[st["idx"][v]]
    q = x @ T[:, :3].T + T[:, 3]
    d = q - y
    if method == "point_to_point":
        return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]), (x, y)
    n = nt[st["idx"][v]]
    if method == "point_to_plane":
        b = np.einsum("ij,ij->i", d, n)
        return b, (np.concatenate([np.cross(q - c, n), n], 1), b)
    m = ns[v] @ T[:, :3].T
    k = len(q)
    M = 2.0 * np.eye(3)[None] - (1.0 - epsilon) * (n[:, :, None] * n[:, None, :] + m[:, :, None] * m[:, None, :])
    A = np.linalg.inv(M) if k else np.zeros((0, 3, 3))
    G = np.concatenate([-GO.skew(q - c), np.tile(np.eye(3), (k, 1, 1))], 2)
    Ad = np.einsum("kij,kj->ki", A, d)
    return np.sqrt(np.maximum(np.einsum("ki,ki->k", d, Ad), 0.0)), (G, A @ G, d)


def _system(method, w, parts):
    """-> (H [6,6], g [6]) of the weighted 6-dof system"""
    if method == "point_to_plane":
        a, b = parts
        return (w[:, None] * a).T @ a, (w[:, None] * a).T @ b
    G, AG, d = parts
    return np.einsum("k,kij,kil->jl", w, G, AG), np.einsum("k,kij,ki->j", w, AG, d)


def icp_robust(method, src, tgt, src_normals, tgt_normals, T0, max_dist, kernel="l2", kernel_k=None, max_iters=30,
               tol_fitness=1e-6, tol_rmse=1e-6, epsilon=GO.EPSILON):
    """One pair; the normals may be None where the method does not use them.  -> the dict of the method's own oracle
    (pivots: the smallest pivot ratio per 6 x 6 solve attempted; cond: per solve that went through) plus w_sum"""
    assert method in METHODS and kernel in KERNELS and (kernel == "l2" or kernel_k > 0)
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    ns = None if src_normals is None else np.asarray(src_normals, np.float64).reshape(-1, 3)
    nt = None if tgt_normals is None else np.asarray(tgt_normals, np.float64).reshape(-1, 3)
    T = np.array(np.asarray(T0, np.float64)[:3], np.float64)
    c = tgt[0] if len(tgt) else np.zeros(3)
    trace = np.full((max_iters + 1, 2), -1.0)
    st = O.evaluate(src, tgt, T, max_dist)
    trace[0] = st["fitness"], st["rmse"]
    margins, deltas, pivots, cond = [(st["gap"], st["edge"])], [], [], []
    k, status, converged = 0, 0, False

    def weigh():
        if st["n_corr"] == 0:
            return np.zeros(0), None
        r, parts = _terms(method, src, tgt, ns, nt, T, st, c, epsilon)
        return weight(kernel, kernel_k, r), parts

    w, parts = weigh()
    while k < max_iters:
        if st["n_corr"] < MIN_CORR[method]:
            status |= 1
            break
        if method == "point_to_point":
            Tn = weighted_kabsch(parts[0], parts[1], w)
            if Tn is not None:
                cond.append(kabsch_cond(parts[0], parts[1], w))
        else:
            H, g = _system(method, w, parts)
            xi, ratio = PO.cholesky_solve(H, g)
            pivots.append(ratio)
            Tn = None if xi is None else (PO.increment(xi, c) @ np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]]))[:3]
            if xi is not None:
                cond.append(np.linalg.cond(H))
        if Tn is None:
            status |= 8
            break
        T = Tn
        k += 1
        new = O.evaluate(src, tgt, T, max_dist)
        df, dr = abs(new["fitness"] - st["fitness"]), abs(new["rmse"] - st["rmse"])
        converged = df < tol_fitness and dr < tol_rmse
        st = new
        w, parts = weigh()
        trace[k] = st["fitness"], st["rmse"]
        margins.append((st["gap"], st["edge"]))
        deltas.append((df, dr))
        if converged:
            break
    if k == max_iters and not converged and (tol_fitness > 0 or tol_rmse > 0):
        status |= 2
    out = {"T": T, "fitness": st["fitness"], "rmse": st["rmse"], "n_corr": st["n_corr"], "iters": k,
           "status": status, "trace": trace, "margins": margins, "deltas": deltas, "pivots": pivots, "cond": cond,
           "w_sum": float(w.sum())}
    return out


def icp_robust_batch(method, frags, normals, pairs, T0, max_dist, kernel="l2", kernel_k=None, max_iters=30,
                     tol_fitness=1e-6, tol_rmse=1e-6, epsilon=GO.EPSILON):
    """The batch as mvr_icp_refine_robust sees it: frags and normals lists of [n_b, 3] (normals None for
    point_to_point); an invalid pair comes out with status 4 and w_sum 0"""
    out = []
    for (s, g), T in zip(np.asarray(pairs).reshape(-1, 2), np.asarray(T0, np.float64)):
        if not (0 <= s < len(frags) and 0 <= g < len(frags)) or not np.all(np.isfinite(T[:3])):
            out.append({"T": T[:3].copy(), "fitness": 0.0, "rmse": 0.0, "n_corr": 0, "iters": 0, "status": 4,
                        "trace": np.full((max_iters + 1, 2), -1.0), "margins": [], "deltas": [], "pivots": [],
                        "cond": [], "w_sum": 0.0})
        else:
            out.append(icp_robust(method, frags[s], frags[g], None if normals is None else normals[s],
                                  None if normals is None else normals[g], T, max_dist, kernel, kernel_k, max_iters,
                                  tol_fitness, tol_rmse, epsilon))
    return out


# --------------------------------------------------------------------------------------------------- the test cases
SCENE_K = {"huber": 0.025, "cauchy": 0.025, "tukey": 0.025, "gm": 0.025 ** 2}      # the scene's voxel size
CONTAMINATED_MAX_DIST, CONTAMINATED_K, CONTAMINATED_ITERS = 0.1, 0.03, 30


def contaminated_case():
    """The corner of icp_plane_oracle.corner_case() as the target; 600 source points drawn from it with 2 mm of noise,
    30 % of them displaced by (0.035, 0.03, 0.04) (about 6 cm: inside max_dist 0.1, a second surface), all mapped by
    the inverse of the case's motion; the start is 1.5 degrees / 4 mm off.  -> (src, tgt, Tt 4x4, T0 4x4)"""
    rng = np.random.default_rng(11)
    tgt = PO.corner_case()[0][0]
    src = tgt[rng.integers(0, 300, 600)] + rng.normal(0, 0.002, (600, 3))
    src[rng.random(600) < 0.3] += np.array([0.035, 0.03, 0.04])
    Tt = O.rigid([1.0, 2.0, -0.5], 25.0, [0.3, -0.2, 0.1])          # source -> target, corner_case's
    Ti = np.linalg.inv(Tt)
    src = src @ Ti[:3, :3].T + Ti[:3, 3]
    T0 = O.perturb(Tt, np.zeros(3), rng, 1.5, 0.004)
    return src, tgt, Tt, T0


def motion_error(T, Tt, tgt):
    """the largest displacement of a target point under T Tt^-1: what the estimate T leaves of the true motion Tt"""
    D = np.concatenate([np.asarray(T, np.float64)[:3], [[0.0, 0.0, 0.0, 1.0]]]) @ np.linalg.inv(Tt)
    return float(np.linalg.norm(tgt @ D[:3, :3].T + D[:3, 3] - tgt, axis=1).max())
