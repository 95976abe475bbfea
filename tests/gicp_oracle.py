"""numpy restatement of the generalized (plane-to-plane) ICP loop (csrc/icp_gicp.hip mvr_icp_refine_generalized), on
top of icp_oracle.evaluate and icp_plane_oracle's Cholesky and increment, and its own test case.

Open3D is absent, so parity is pinned to the semantics stated here (include/mvreg.h) and to ground
truth.  A point with unit normal n has covariance C = I - (1 - eps) n n^T: 1 in the surface, eps along the normal.

    loop:     state = eval(T0)                                       (icp_oracle.evaluate: Euclidean fitness / rmse)
              for k in 1..max_iters:
                  if state.n_corr < 6: status |= 1; break
                  q = T x, y = its match, n = the normal of y, m = R n_s (n_s the normal of x, R the rotation of T),
                  c = the target's first point
                  M = 2 I - (1 - eps)(n n^T + m m^T), A = M^-1;  G = [-[q - c]x | I], d = q - y
                  H = sum G^T A G, g = sum G^T A d
                  Cholesky of H; a pivot that fails pivot > 1e-12 max H_ii: status |= 8; break (T kept)
                  xi = -H^-1 g;  R_inc = Rz(xi2) Ry(xi1) Rx(xi0);  T <- [R_inc | xi[3:6] + c - R_inc c] T
                  new = eval(T); converged / state / status 2 / status 4 as icp_oracle.icp

The results carry the margins of icp_plane_oracle.icp_plane: nearest-neighbour gap and |d - max_dist| per evaluation,
the stopping deltas, the smallest pivot ratio and cond(H) per solve.
"""
import numpy as np

import icp_oracle as O
import icp_plane_oracle as PO

EPSILON = 1e-3


def skew(w):
    """[w]x per row: [n,3] -> [n,3,3]"""
    S = np.zeros((len(w), 3, 3))
    S[:, 0, 1], S[:, 0, 2] = -w[:, 2], w[:, 1]
    S[:, 1, 0], S[:, 1, 2] = w[:, 2], -w[:, 0]
    S[:, 2, 0], S[:, 2, 1] = -w[:, 1], w[:, 0]
    return S


def system(q, y, n, m, c, epsilon):
    """-> (H [6,6], g [6]) of the matched rows: q = T x, y the matches, n their normals, m = R n_s, c the origin"""
    k = len(q)
    M = 2.0 * np.eye(3)[None] - (1.0 - epsilon) * (n[:, :, None] * n[:, None, :] + m[:, :, None] * m[:, None, :])
    A = np.linalg.inv(M) if k else np.zeros((0, 3, 3))
    G = np.concatenate([-skew(q - c), np.tile(np.eye(3), (k, 1, 1))], 2)
    AG = A @ G
    H = np.einsum("kij,kil->jl", G, AG)
    g = np.einsum("kij,ki->j", AG, q - y)
    return H, g


def gicp(src, tgt, src_normals, tgt_normals, T0, max_dist, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6,
         epsilon=EPSILON):
    """One pair; src_normals [n,3], tgt_normals [m,3].  -> icp_plane_oracle.icp_plane's dict"""
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    ns = np.asarray(src_normals, np.float64).reshape(-1, 3)
    nt = np.asarray(tgt_normals, np.float64).reshape(-1, 3)
    T = np.array(np.asarray(T0, np.float64)[:3], np.float64)
    c = tgt[0] if len(tgt) else np.zeros(3)
    trace = np.full((max_iters + 1, 2), -1.0)
    st = O.evaluate(src, tgt, T, max_dist)
    trace[0] = st["fitness"], st["rmse"]
    margins, deltas, pivots, cond = [(st["gap"], st["edge"])], [], [], []
    k, status, converged = 0, 0, False
    while k < max_iters:
        if st["n_corr"] < 6:
            status |= 1
            break
        v = st["valid"]
        q = src[v] @ T[:, :3].T + T[:, 3]
        H, g = system(q, tgt[st["idx"][v]], nt[st["idx"][v]], ns[v] @ T[:, :3].T, c, epsilon)
        xi, ratio = PO.cholesky_solve(H, g)
        pivots.append(ratio)
        if xi is None:
            status |= 8
            break
        cond.append(np.linalg.cond(H))
        T = (PO.increment(xi, c) @ np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]]))[:3]
        k += 1
        new = O.evaluate(src, tgt, T, max_dist)
        df, dr = abs(new["fitness"] - st["fitness"]), abs(new["rmse"] - st["rmse"])
        converged = df < tol_fitness and dr < tol_rmse
        st = new
        trace[k] = st["fitness"], st["rmse"]
        margins.append((st["gap"], st["edge"]))
        deltas.append((df, dr))
        if converged:
            break
    if k == max_iters and not converged and (tol_fitness > 0 or tol_rmse > 0):
        status |= 2
    return {"T": T, "fitness": st["fitness"], "rmse": st["rmse"], "n_corr": st["n_corr"], "iters": k,
            "status": status, "trace": trace, "margins": margins, "deltas": deltas, "pivots": pivots, "cond": cond}


def gicp_batch(frags, normals, pairs, T0, max_dist, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6, epsilon=EPSILON):
    """The batch as mvr_icp_refine_generalized sees it: frags and normals lists of [n_b, 3]; an invalid pair comes out
    with status 4"""
    out = []
    for (s, g), T in zip(np.asarray(pairs).reshape(-1, 2), np.asarray(T0, np.float64)):
        if not (0 <= s < len(frags) and 0 <= g < len(frags)) or not np.all(np.isfinite(T[:3])):
            out.append({"T": T[:3].copy(), "fitness": 0.0, "rmse": 0.0, "n_corr": 0, "iters": 0, "status": 4,
                        "trace": np.full((max_iters + 1, 2), -1.0), "margins": [], "deltas": [], "pivots": [],
                        "cond": []})
        else:
            out.append(gicp(frags[s], frags[g], normals[s], normals[g], T, max_dist, max_iters, tol_fitness, tol_rmse,
                            epsilon))
    return out


# --------------------------------------------------------------------------------------------------- the test cases
EPSILONS = (EPSILON, 1.0, 1e-2)        # the default, the isotropic limit, one between
LINE_MAX_DIST = 0.1


def line_case():
    """corner_case() plus a source of 9 points on an axis-parallel line (y = 0.01, z = 0) against the planar target,
    T0 = I: a rotation about the line moves nothing, so H's first pivot is 0 whatever the covariances.
    -> (frags, pairs [P,2], T0 [P,4,4], row of the line pair)"""
    frags, pairs, T0 = PO.corner_case()
    line = np.zeros((9, 3))
    line[:, 0], line[:, 1] = np.linspace(-0.2, 0.2, 9), 0.01
    frags = frags + [line]
    pairs = np.concatenate([pairs, [[len(frags) - 1, 1]]])
    T0 = np.concatenate([T0, np.eye(4)[None]])
    return frags, pairs, T0, len(pairs) - 1
