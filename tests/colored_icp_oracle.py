"""numpy restatement of the colour gradients (csrc/color_grad.hip mvr_color_gradient), of the voxel colours
(csrc/overlap.hip mvr_voxel_centroids_colored) and of the coloured ICP loop (csrc/icp_colored.hip
mvr_icp_refine_colored), on top of icp_oracle.evaluate, icp_plane_oracle.cholesky_solve / increment and
icp_robust_oracle.weight, and their test cases.

Open3D is absent, so parity is pinned to the semantics stated here (include/mvreg.h) and to ground
truth.  The neighbour search is sklearn's kd-tree in fp64 and every sum numpy's; the kernels walk a cell hash and sum
in its order.

    intensity:  I = (c0 + c1 + c2) / 3.0
    gradient:   the neighbours of x_i are the points of its fragment with |x_j - x_i| < radius (strict; x_i itself is
                one); fewer than 4: 0; else with n the normal of i (as given), e = x_j - x_i, u = e - (e . n) n:
                A = sum u u^T + (n_nbr - 1)^2 n n^T, h = sum u (I_j - I_i), A d = h by Cholesky; a pivot that fails
                pivot > 1e-12 max A_ii, or a solution that is not finite: 0
    loop:       state = eval(T0)                                     (icp_oracle.evaluate: Euclidean fitness / rmse)
                for k in 1..max_iters:
                    if state.n_corr < 6: status |= 1; break
                    q = T x_i, y = its match t, n / d the normal / gradient of t, c = the target's first point
                    e = q - y; g = e . n; r_I = I_s[i] - (I_t[t] + d . (e - g n)); dM = -(d - (d . n) n)
                    J_G = [(q - c) x n, n], J_I = [(q - c) x dM, dM]
                    w_G = w(sqrt(lambda) g), w_I = w(sqrt(1 - lambda) r_I)
                    H = sum lambda w_G J_G J_G^T + (1 - lambda) w_I J_I J_I^T
                    b = sum lambda w_G J_G g + (1 - lambda) w_I J_I r_I
                    Cholesky of H; a failed pivot: status |= 8; break (T kept)
                    xi = -H^-1 b; T <- increment(xi, c) T; new = eval(T); converged / status 2 / 4 as icp_oracle.icp
                w_sum = sum (lambda w_G + (1 - lambda) w_I) at the returned T

Besides the results every function reports the margins a comparison rests on: per point the smallest
| |x_j - x_i| - radius | and the smallest 3 x 3 pivot / max A_ii; per solve the smallest 6 x 6 pivot / max H_ii, and
icp_oracle's nearest-neighbour gap, |d - max_dist| and stopping deltas.
"""
import functools

import numpy as np

import icp_oracle as O
import icp_plane_oracle as PO
import icp_robust_oracle as RO

PIVOT_FLOOR = 1e-12
LAMBDA = 0.968


def intensity(colors):
    c = np.asarray(colors, np.float64).reshape(-1, 3)
    return (c[:, 0] + c[:, 1] + c[:, 2]) / 3.0


# ---------------------------------------------------------------------------------------------------- voxel colours
def voxel_colors(xyz, colors, voxel):
    """Open3D's voxel_down_sample of one fragment with colours, both through float32 as the library takes them.
    -> (centroids [k,3], mean colours [k,3]), fp64 sums in input order, the voxels ordered by (x, y, z) index: the row
    order of FragmentOverlap(.., 'FCGF')"""
    p = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    c = np.asarray(colors, np.float64).astype(np.float32).astype(np.float64).reshape(-1, 3)
    if len(p) == 0:
        return p, c
    idx = np.floor((p - (p.min(0) - voxel * 0.5)) / voxel).astype(np.int64)
    _, inv = np.unique(idx, axis=0, return_inverse=True)          # rows sorted lexicographically
    inv = inv.reshape(-1)
    k = inv.max() + 1
    sp, sc = np.zeros((k, 3)), np.zeros((k, 3))
    np.add.at(sp, inv, p)                                         # unbuffered: in input order
    np.add.at(sc, inv, c)
    cnt = np.bincount(inv, minlength=k).astype(np.float64)[:, None]
    return sp / cnt, sc / cnt


# -------------------------------------------------------------------------------------------------------- gradients
def cholesky3(A, h):
    """-> (d = A^-1 h or None when a pivot fails pivot > PIVOT_FLOOR max A_ii, smallest pivot / max A_ii seen)"""
    top = max(np.max(np.diag(A)), 0.0)
    L = np.zeros((3, 3))
    ratio = np.inf
    for j in range(3):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        ratio = min(ratio, d / top if top > 0 else 0.0)
        if not d > PIVOT_FLOOR * top:
            return None, ratio
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 3):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(3)
    for i in range(3):
        y[i] = (h[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(3)
    for i in range(2, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x, ratio


def color_gradients(pts, normals, colors, radius):
    """One fragment.  -> dict(intensity [n], grad [n,3], n_nbr [n], edge [n] (smallest | d - radius | over the
    fragment's other points, looked for up to 1.25 radius and capped at 0.25 radius), pivot [n] (the smallest pivot
    ratio of the 3 x 3 solve, inf below 4 neighbours), nan [n] (a colour of the ball is not finite))"""
    from sklearn.neighbors import NearestNeighbors
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    normals = np.asarray(normals, np.float64).reshape(-1, 3)
    n = len(pts)
    I = intensity(colors)
    out = {"intensity": I, "grad": np.zeros((n, 3)), "n_nbr": np.zeros(n, np.int32),
           "edge": np.full(n, 0.25 * radius), "pivot": np.full(n, np.inf), "nan": np.zeros(n, bool)}
    if n == 0:
        return out
    nbrs = NearestNeighbors(algorithm="kd_tree").fit(pts).radius_neighbors(pts, 1.25 * radius, return_distance=False)
    for i in range(n):
        e = pts[nbrs[i]] - pts[i]
        d = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        out["edge"][i] = min(out["edge"][i], np.abs(d - radius).min())
        rows = nbrs[i][d < radius]
        e = e[d < radius]
        k = len(e)
        out["n_nbr"][i] = k
        out["nan"][i] = not np.isfinite(I[rows]).all()
        if k < 4:
            continue
        nv = normals[i]
        u = e - (e @ nv)[:, None] * nv
        A = u.T @ u + float(k - 1) ** 2 * np.outer(nv, nv)
        with np.errstate(invalid="ignore"):
            h = u.T @ (I[rows] - I[i])
        sol, out["pivot"][i] = cholesky3(A, h)
        if sol is not None and np.isfinite(sol).all():
            out["grad"][i] = sol
    return out


def color_gradients_batch(frags, normals, colors, radius):
    """-> a list of color_gradients() dicts, one per fragment"""
    return [color_gradients(f, normals[b], colors[b], radius) for b, f in enumerate(frags)]


def near_floor(pivot):
    """the points a comparison may leave out: the oracle's pivot ratio lies within 100 x of the floor"""
    return (pivot > PIVOT_FLOOR / 100.0) & (pivot < PIVOT_FLOOR * 100.0)


# ------------------------------------------------------------------------------------------------------------- loop
def _system(src, tgt, nt, I_s, I_t, g_t, T, st, c, lam, kernel, kernel_k):
    """the 6 x 6 system of state st at T -> (H, b, w_sum)"""
    v = st["valid"]
    idx = st["idx"][v]
    q = src[v] @ T[:, :3].T + T[:, 3]
    y, n, d = tgt[idx], nt[idx], g_t[idx]
    e = q - y
    g = np.einsum("ij,ij->i", e, n)
    r_i = I_s[v] - (I_t[idx] + np.einsum("ij,ij->i", d, e - g[:, None] * n))
    dM = -(d - np.einsum("ij,ij->i", d, n)[:, None] * n)
    JG = np.concatenate([np.cross(q - c, n), n], 1)
    JI = np.concatenate([np.cross(q - c, dM), dM], 1)
    wG = RO.weight(kernel, kernel_k, np.sqrt(lam) * g)
    wI = RO.weight(kernel, kernel_k, np.sqrt(1.0 - lam) * r_i)
    H = lam * (wG[:, None] * JG).T @ JG + (1.0 - lam) * (wI[:, None] * JI).T @ JI
    b = lam * (wG[:, None] * JG).T @ g + (1.0 - lam) * (wI[:, None] * JI).T @ r_i
    return H, b, float((lam * wG + (1.0 - lam) * wI).sum())


def colored_icp(src, tgt, tgt_normals, src_intensity, tgt_intensity, tgt_grad, T0, max_dist, lambda_geometric=LAMBDA,
                kernel="l2", kernel_k=None, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6):
    """One pair.  -> icp_plane_oracle.icp_plane's dict (pivots: the smallest pivot ratio per solve attempted; cond:
    per solve that went through) plus w_sum"""
    assert kernel in RO.KERNELS and (kernel == "l2" or kernel_k > 0) and 0.0 <= lambda_geometric <= 1.0
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    nt = np.asarray(tgt_normals, np.float64).reshape(-1, 3)
    I_s, I_t = np.asarray(src_intensity, np.float64).reshape(-1), np.asarray(tgt_intensity, np.float64).reshape(-1)
    g_t = np.asarray(tgt_grad, np.float64).reshape(-1, 3)
    T = np.array(np.asarray(T0, np.float64)[:3], np.float64)
    c = tgt[0] if len(tgt) else np.zeros(3)
    trace = np.full((max_iters + 1, 2), -1.0)
    st = O.evaluate(src, tgt, T, max_dist)
    trace[0] = st["fitness"], st["rmse"]
    margins, deltas, pivots, cond = [(st["gap"], st["edge"])], [], [], []
    k, status, converged = 0, 0, False

    def system():
        if st["n_corr"] == 0:
            return None, None, 0.0
        return _system(src, tgt, nt, I_s, I_t, g_t, T, st, c, lambda_geometric, kernel, kernel_k)

    H, b, w_sum = system()
    while k < max_iters:
        if st["n_corr"] < 6:
            status |= 1
            break
        xi, ratio = PO.cholesky_solve(H, b)
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
        H, b, w_sum = system()
        trace[k] = st["fitness"], st["rmse"]
        margins.append((st["gap"], st["edge"]))
        deltas.append((df, dr))
        if converged:
            break
    if k == max_iters and not converged and (tol_fitness > 0 or tol_rmse > 0):
        status |= 2
    return {"T": T, "fitness": st["fitness"], "rmse": st["rmse"], "n_corr": st["n_corr"], "iters": k,
            "status": status, "trace": trace, "margins": margins, "deltas": deltas, "pivots": pivots, "cond": cond,
            "w_sum": w_sum}


def colored_icp_batch(frags, normals, intensities, grads, pairs, T0, max_dist, lambda_geometric=LAMBDA, kernel="l2",
                      kernel_k=None, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6):
    """The batch as mvr_icp_refine_colored sees it: frags, normals, intensities and grads lists per fragment; an
    invalid pair comes out with status 4 and w_sum 0"""
    out = []
    for (s, g), T in zip(np.asarray(pairs).reshape(-1, 2), np.asarray(T0, np.float64)):
        if not (0 <= s < len(frags) and 0 <= g < len(frags)) or not np.all(np.isfinite(T[:3])):
            out.append({"T": T[:3].copy(), "fitness": 0.0, "rmse": 0.0, "n_corr": 0, "iters": 0, "status": 4,
                        "trace": np.full((max_iters + 1, 2), -1.0), "margins": [], "deltas": [], "pivots": [],
                        "cond": [], "w_sum": 0.0})
        else:
            out.append(colored_icp(frags[s], frags[g], normals[g], intensities[s], intensities[g], grads[g], T,
                                   max_dist, lambda_geometric, kernel, kernel_k, max_iters, tol_fitness, tol_rmse))
    return out


# --------------------------------------------------------------------------------------------------- the test cases
FIELD_K = np.array([[9.0, 4.0, -3.0], [-5.0, 8.0, 6.0], [3.0, -7.0, 10.0]])
FIELD_PHI = np.array([0.3, 1.1, 2.0])
ROBUST_K = 0.025


def color_field(world):
    """the scene's colours: 0.5 + 0.4 sin(K w + phi) of the world position w, the same for every fragment that sees
    the point"""
    return 0.5 + 0.4 * np.sin(np.asarray(world, np.float64) @ FIELD_K.T + FIELD_PHI)


@functools.lru_cache(maxsize=None)
def scene4_raw_colors():
    """the colours of icp_oracle.scene4()'s raw points: the field at their world positions pose_b x"""
    raw, poses = O.scene4()
    return [color_field(np.asarray(f, np.float64) @ poses[b][:3, :3].T + poses[b][:3, 3]) for b, f in enumerate(raw)]


@functools.lru_cache(maxsize=None)
def scene4_colored_centroids():
    """(centroids, mean colours) per fragment of the scene at voxel 0.025, in FragmentOverlap's row order"""
    both = [voxel_colors(f, c, 0.025) for f, c in zip(O.scene4()[0], scene4_raw_colors())]
    return [b[0] for b in both], [b[1] for b in both]


@functools.lru_cache(maxsize=None)
def scene4_inputs(radius=PO.NORMAL_RADIUS):
    """the oracle's own inputs of the scene's loop cases: (centroids, normals, intensities, gradients) per fragment,
    normals and gradients over `radius`"""
    cent, col = scene4_colored_centroids()
    nrm = [r["normals"] for r in PO.estimate_normals_batch(cent, radius)]
    gr = color_gradients_batch(cent, nrm, col, radius)
    return cent, nrm, [g["intensity"] for g in gr], [g["grad"] for g in gr]


def linear_field_case(tilted=False, seed=8, n=4000):
    """4000 random points of a 1 m square in a plane and an exactly linear intensity I = 0.3 + a . x on them.  The
    plane is z = 0.3, or tilted by 33 degrees: with the normal along an axis the row (n_nbr - 1) n . d = 0, thousands
    of times heavier than the tangent rows, stays in a block of its own and the solve is exact to a few eps; tilted it
    enters every entry of A, and the Cholesky loses the digits of A's condition, about 1 / the pivot ratio.
    -> (points, the plane's unit normal, grey colours [n,3], a)"""
    rng = np.random.default_rng(seed)
    R = O.rigid([0.4, -1.0, 0.7], 33.0, np.zeros(3))[:3, :3] if tilted else np.eye(3)
    ab = rng.uniform(-0.5, 0.5, (n, 2))
    pts = ab[:, :1] * R[:, 0] + ab[:, 1:] * R[:, 1] + np.array([0.2, -0.1, 0.3])
    a = np.array([0.31, -0.22, 0.27])
    I = 0.3 + pts @ a
    return pts, R[:, 2].copy(), np.repeat(I[:, None], 3, 1), a


SMALL_NAN = (7, 10)                    # small_colored_case: fragment and row of the NaN colour
SMALL_FOUR, SMALL_LINE = 8, 9          # its 4-point and collinear fragments


def small_colored_case(seed=9):
    """icp_plane_oracle.small_normals_case() with the field's colours, a 4-point fragment and 64 collinear points
    (both in the same region around the origin), and one NaN colour in the 1025-point cloud
    -> (frags, colors)"""
    rng = np.random.default_rng(seed)
    frags = list(PO.small_normals_case())
    frags.append(rng.uniform(-0.015, 0.015, (4, 3)))
    u = np.array([0.6, -0.3, 0.74])
    frags.append(np.linspace(-0.16, 0.16, 64)[:, None] * (u / np.linalg.norm(u)) + np.array([0.01, 0.02, -0.01]))
    colors = [color_field(f) for f in frags]
    colors[SMALL_NAN[0]][SMALL_NAN[1], 1] = np.nan
    return frags, colors


def corner_colors(frags):
    """icp_plane_oracle.corner_case()'s fragments coloured for the status bits: the field at T_true x for the sources
    of the corner (so that both sides of a match see the same colour), the field itself on the corner, and one
    constant colour on the planar target, whose gradients are then exactly 0: its pair stays degenerate (status 8)"""
    Tt = O.rigid([1.0, 2.0, -0.5], 25.0, [0.3, -0.2, 0.1])
    colors = [color_field(frags[0]), np.full((len(frags[1]), 3), 0.5)]
    for f in frags[2:-1]:
        colors.append(color_field(np.asarray(f, np.float64).reshape(-1, 3) @ Tt[:3, :3].T + Tt[:3, 3]))
    colors.append(color_field(frags[-1]))
    return colors


PLANE_RADIUS, PLANE_ITERS = 0.075, 30


@functools.lru_cache(maxsize=None)
def textured_plane_case(seed=0):
    """The case colour exists for: 2000 uniform points of a 1 m square as the source, an independent sampling of 4000
    points of a 1.2 m square as the target, the plane tilted 25 degrees about (1, 2, 0.5), the target moved in its
    plane by 3 degrees about the normal and by (0.02, -0.015); grey texture 0.5 + 0.2 sin(7x + 2y) + 0.2 cos(-3x + 6y)
    of the plane's own coordinates.  The start is the identity.
    -> (src, src_colors, tgt, tgt_colors, T_true 4x4 with x_target ~ T_true x_source)"""
    rng = np.random.default_rng(seed)

    def tex(p):
        return 0.5 + 0.2 * np.sin(7.0 * p[:, 0] + 2.0 * p[:, 1]) + 0.2 * np.cos(-3.0 * p[:, 0] + 6.0 * p[:, 1])

    s = np.zeros((2000, 3))
    s[:, :2] = rng.uniform(-0.5, 0.5, (2000, 2))
    t = np.zeros((4000, 3))
    t[:, :2] = rng.uniform(-0.6, 0.6, (4000, 2))
    tilt = O.rigid([1.0, 2.0, 0.5], 25.0, np.zeros(3))
    move = O.rigid([0.0, 0.0, 1.0], 3.0, [0.02, -0.015, 0.0])
    Tt = tilt @ move @ np.linalg.inv(tilt)
    to_tgt = tilt @ move
    src = s @ tilt[:3, :3].T
    tgt = t @ to_tgt[:3, :3].T + to_tgt[:3, 3]
    return src, np.repeat(tex(s)[:, None], 3, 1), tgt, np.repeat(tex(t)[:, None], 3, 1), Tt


def motion_error(T, Tt, src):
    """the largest distance between T x and Tt x over the source points"""
    src = np.asarray(src, np.float64)
    T, Tt = np.asarray(T, np.float64)[:3], np.asarray(Tt, np.float64)[:3]
    return float(np.linalg.norm(src @ (T[:, :3] - Tt[:, :3]).T + (T[:, 3] - Tt[:, 3]), axis=1).max())
