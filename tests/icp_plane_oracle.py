"""numpy restatement of the normal estimation (csrc/normals.hip mvr_estimate_normals) and of the point-to-plane ICP
loop (csrc/icp_plane.hip mvr_icp_refine_plane), on top of icp_oracle.evaluate, and their test cases.

Open3D is absent, so parity is pinned to the semantics stated here (include/mvreg.h) and to ground
truth.  The neighbour search is sklearn's kd-tree in fp64 and the eigen-solve np.linalg.eigh; the kernel walks a cell
hash and solves with a cyclic Jacobi.

    normals:  the neighbours of x_i are the points of its fragment with |x_j - x_i| < radius (strict; x_i itself is
              one); fewer than 3: (0, 0, 1); else C = mean(e e^T) - mean(e) mean(e)^T over e = x_j - x_i and the normal
              is the unit eigenvector of C's smallest eigenvalue, flipped towards the viewpoint when one is given
    loop:     state = eval(T0)                                       (icp_oracle.evaluate: Euclidean fitness / rmse)
              for k in 1..max_iters:
                  if state.n_corr < 6: status |= 1; break
                  q = T x, y = its match, n = the normal of y, c = the target's first point
                  a = [(q - c) x n, n], b = (q - y) . n;  H = sum a a^T, g = sum a b
                  Cholesky of H; a pivot that fails pivot > 1e-12 max H_ii: status |= 8; break (T kept)
                  xi = -H^-1 g;  R_inc = Rz(xi2) Ry(xi1) Rx(xi0);  T <- [R_inc | xi[3:6] + c - R_inc c] T
                  new = eval(T); converged / state / status 2 / status 4 as icp_oracle.icp

Besides the results every function reports the margins a comparison rests on: per point the smallest
| |x_j - x_i| - radius | and the relative eigen-gap (l1 - l0) / l2; per solve the smallest pivot / max H_ii; and
icp_oracle's nearest-neighbour gap, |d - max_dist| and stopping deltas.
"""
import functools

import numpy as np

import icp_oracle as O

PIVOT_FLOOR = 1e-12


# ---------------------------------------------------------------------------------------------------------- normals
def estimate_normals(pts, radius, viewpoint=None):
    """One fragment.  -> dict(normals [n,3], n_nbr [n], edge [n] (smallest | d - radius | over the fragment's other
    points, looked for up to 1.25 radius and capped at 0.25 radius), gap [n] ((l1 - l0) / l2, inf below 3
    neighbours or for l2 = 0))"""
    from sklearn.neighbors import NearestNeighbors
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    out = {"normals": np.tile([0.0, 0.0, 1.0], (n, 1)), "n_nbr": np.zeros(n, np.int32),
           "edge": np.full(n, 0.25 * radius), "gap": np.full(n, np.inf)}
    if n == 0:
        return out
    nbrs = NearestNeighbors(algorithm="kd_tree").fit(pts).radius_neighbors(pts, 1.25 * radius, return_distance=False)
    for i in range(n):
        e = pts[nbrs[i]] - pts[i]
        d = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        out["edge"][i] = min(out["edge"][i], np.abs(d - radius).min())
        e = e[d < radius]
        out["n_nbr"][i] = len(e)
        if len(e) < 3:
            continue
        m = e.mean(0)
        C = e.T @ e / len(e) - np.outer(m, m)
        w, v = np.linalg.eigh(C)
        out["normals"][i] = v[:, 0] / np.linalg.norm(v[:, 0])
        if w[2] > 0:
            out["gap"][i] = (w[1] - w[0]) / w[2]
    if viewpoint is not None:
        flip = np.einsum("ij,ij->i", out["normals"], np.asarray(viewpoint, np.float64) - pts) < 0
        out["normals"][flip] *= -1.0
    return out


def estimate_normals_batch(frags, radius, viewpoints=None):
    """-> a list of estimate_normals() dicts, one per fragment"""
    return [estimate_normals(f, radius, None if viewpoints is None else viewpoints[b]) for b, f in enumerate(frags)]


# ------------------------------------------------------------------------------------------------------------- loop
def cholesky_solve(H, g):
    """-> (xi = -H^-1 g or None when a pivot fails pivot > PIVOT_FLOOR max H_ii, smallest pivot / max H_ii seen)"""
    top = max(np.max(np.diag(H)), 0.0)
    L = np.zeros((6, 6))
    ratio = np.inf
    for j in range(6):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        ratio = min(ratio, d / top if top > 0 else 0.0)
        if not d > PIVOT_FLOOR * top:
            return None, ratio
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - L[i, :i] @ y[:i]) / L[i, i]
    xi = np.zeros(6)
    for i in range(5, -1, -1):
        xi[i] = (y[i] - L[i + 1:, i] @ xi[i + 1:]) / L[i, i]
    return xi, ratio


def increment(xi, c):
    """[Rz(xi2) Ry(xi1) Rx(xi0) | xi[3:6] + c - R c] as 4x4 (Open3D's TransformVector6dToMatrix4d about c)"""
    cx, sx, cy, sy, cz, sz = np.cos(xi[0]), np.sin(xi[0]), np.cos(xi[1]), np.sin(xi[1]), np.cos(xi[2]), np.sin(xi[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    D = np.eye(4)
    D[:3, :3] = Rz @ Ry @ Rx
    D[:3, 3] = xi[3:] + c - D[:3, :3] @ c
    return D


def icp_plane(src, tgt, normals, T0, max_dist, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6, solver="cholesky"):
    """One pair; normals [m,3] of the target.  -> icp_oracle.icp's dict plus pivots [smallest pivot ratio per solve
    attempted] and cond [cond(H) per solve].  solver 'lstsq' replaces the Cholesky (no degeneracy test): a check of
    the oracle's own solve."""
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    normals = np.asarray(normals, np.float64).reshape(-1, 3)
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
        q = src[st["valid"]] @ T[:, :3].T + T[:, 3]
        y, n = tgt[st["idx"][st["valid"]]], normals[st["idx"][st["valid"]]]
        a = np.concatenate([np.cross(q - c, n), n], 1)
        b = np.einsum("ij,ij->i", q - y, n)
        H, g = a.T @ a, a.T @ b
        if solver == "lstsq":
            xi = np.linalg.lstsq(a, -b, rcond=None)[0]
        else:
            xi, ratio = cholesky_solve(H, g)
            pivots.append(ratio)
            if xi is None:
                status |= 8
                break
        cond.append(np.linalg.cond(H))
        T = (increment(xi, c) @ np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]]))[:3]
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


def icp_plane_batch(frags, normals, pairs, T0, max_dist, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6):
    """The batch as mvr_icp_refine_plane sees it: frags and normals lists of [n_b, 3]; an invalid pair comes out with
    status 4"""
    out = []
    for (s, g), T in zip(np.asarray(pairs).reshape(-1, 2), np.asarray(T0, np.float64)):
        if not (0 <= s < len(frags) and 0 <= g < len(frags)) or not np.all(np.isfinite(T[:3])):
            out.append({"T": T[:3].copy(), "fitness": 0.0, "rmse": 0.0, "n_corr": 0, "iters": 0, "status": 4,
                        "trace": np.full((max_iters + 1, 2), -1.0), "margins": [], "deltas": [], "pivots": [],
                        "cond": []})
        else:
            out.append(icp_plane(frags[s], frags[g], normals[g], T, max_dist, max_iters, tol_fitness, tol_rmse))
    return out


def pivot_range(results):
    """(smallest pivot ratio of a solve that went through, largest of one that was refused) over the results"""
    good = [p for r in results for p in (r["pivots"][:-1] if r["status"] & 8 else r["pivots"])]
    bad = [r["pivots"][-1] for r in results if r["status"] & 8]
    return min(good + [np.inf]), max(bad + [-np.inf])


# --------------------------------------------------------------------------------------------------- the test cases
NORMAL_RADIUS = 0.075        # the scene's normals: the index's cell
SHIFT = np.array([100.0, -200.0, 50.0])


@functools.lru_cache(maxsize=None)
def scene4_normals(radius=NORMAL_RADIUS):
    """estimate_normals of the scene's centroids (the oracle's own row order)"""
    return estimate_normals_batch(O.scene4_centroids(), radius)


def conjugate_starts(T, shift):
    """the transforms of a scene whose every fragment is moved by `shift`: x' = x + shift on both sides"""
    T = np.array(T, np.float64)
    for k in range(len(T)):
        T[k, :3, 3] = T[k, :3, 3] + shift - T[k, :3, :3] @ shift
    return T


SMALL_SIZES = O.SMALL_SIZES            # 0, 1, 2, 3, 63, 64, 65, 1025
SMALL_R_INDEX = 0.1
PLANAR = 5                             # the fragment of small_normals_case that lies in the plane z = 0


def small_normals_case(seed=4):
    """Fragments of SMALL_SIZES points for an index of cell SMALL_R_INDEX, all in the same region around the origin
    (a neighbour leaked from another fragment changes n_nbr): the 1- and 2-point fragments (normal (0, 0, 1)), three
    points of a triangle, jittered tilted planes of 63 and 65 points, 64 points exactly in z = 0, and a 1025-point
    cloud of three slabs a third of which has one coordinate on a cell face."""
    rng = np.random.default_rng(seed)

    def slab(n, normal, jitter, half=0.15):
        normal = np.asarray(normal, np.float64) / np.linalg.norm(normal)
        u = np.cross(normal, [0.3, -0.5, 0.8])
        u /= np.linalg.norm(u)
        w = np.cross(normal, u)
        ab = rng.uniform(-half, half, (n, 2))
        return ab[:, :1] * u + ab[:, 1:] * w + rng.normal(0, jitter, (n, 1)) * normal

    frags = [np.zeros((0, 3)), rng.uniform(-0.02, 0.02, (1, 3)), rng.uniform(-0.03, 0.03, (2, 3)),
             rng.uniform(-0.04, 0.04, (3, 3)), slab(63, [1.0, 2.0, 3.0], 0.002)]
    flat = np.zeros((64, 3))
    flat[:, :2] = rng.uniform(-0.15, 0.15, (64, 2))
    frags.append(flat)
    frags.append(slab(65, [-2.0, 1.0, 0.5], 0.002))
    big = np.concatenate([slab(341, [0.0, 0.0, 1.0], 0.003, 0.25), slab(342, [1.0, 0.0, 0.0], 0.003, 0.25),
                          slab(342, [0.0, 1.0, 0.0], 0.003, 0.25)])
    axis = rng.integers(0, 3, 341)
    big[np.arange(341) * 3, axis] = np.round(big[np.arange(341) * 3, axis] / SMALL_R_INDEX) * SMALL_R_INDEX
    frags.append(big[rng.permutation(len(big))])
    assert tuple(len(f) for f in frags) == SMALL_SIZES
    return frags


def small_normals_pairs(seed=6):
    """Pairs and starts on small_normals_case for the searches that share one core: every fragment as the source
    against the 1025-point cloud (itself included) and that cloud against every other fragment, each from the identity
    perturbed by 1.5 degrees and sigma 4 mm, so that no distance is zero.  -> (pairs [15,2], T0 [15,4,4])"""
    rng = np.random.default_rng(seed)
    big = len(SMALL_SIZES) - 1
    pairs = [(s, big) for s in range(big + 1)] + [(big, t) for t in range(big)]
    T0 = [O.perturb(np.eye(4), np.zeros(3), rng, 1.5, 0.004) for _ in pairs]
    return np.asarray(pairs), np.asarray(T0)


CORNER_RADIUS = 0.1                    # cell, normal radius and max_dist of corner_case


def corner_case(seed=5):
    """Raw-point fragments for FragmentOverlap(.., '3DMatch', radius=CORNER_RADIUS): fragment 0 a corner of three
    orthogonal jittered faces (300 points, the faces interleaved row by row), fragment 1 a 200-point target exactly in
    the plane z = 0; then sources of SMALL_SIZES' counterpart (0, 1, 5, 6, 63, 64, 65, 1025 jittered corner points
    moved by a known motion) against the corner, a far-away source, and a source against the planar target.
    -> (frags, pairs [P,2], T0 [P,4,4])"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0.0, 0.4, (300, 2))
    w = rng.normal(0, 0.002, 300)
    tgt = np.empty((300, 3))
    for k in range(3):      # face k is normal to axis k
        rows = np.arange(k, 300, 3)
        tgt[rows, k] = w[rows]
        tgt[rows, (k + 1) % 3], tgt[rows, (k + 2) % 3] = uv[rows, 0], uv[rows, 1]
    tgt -= 0.15             # straddles zero
    flat = np.zeros((200, 3))
    flat[:, :2] = rng.uniform(-0.3, 0.3, (200, 2))
    Tt = O.rigid([1.0, 2.0, -0.5], 25.0, [0.3, -0.2, 0.1])          # source -> target
    Ti = np.linalg.inv(Tt)
    frags, pairs, T0 = [tgt, flat], [], []
    for n in (0, 1, 5, 6, 63, 64, 65, 1025):
        pick = np.arange(n) % 300 if n <= 300 else rng.integers(0, 300, n)
        p = tgt[pick] + rng.normal(0, 0.003, (n, 3))
        frags.append(p @ Ti[:3, :3].T + Ti[:3, 3])
        pairs.append((len(frags) - 1, 0))
        T0.append(O.perturb(Tt, np.zeros(3), rng, 1.5, 0.004))
    frags.append(tgt[:40] + 100.0)                                   # no correspondence at the start
    pairs.append((len(frags) - 1, 0))
    T0.append(np.eye(4))
    frags.append(flat[:80] + rng.normal(0, 0.004, (80, 3)))          # against the plane: H has zero rows
    pairs.append((len(frags) - 1, 1))
    T0.append(O.rigid([0.2, 0.1, 1.0], 1.0, [0.003, -0.002, 0.004]))
    return frags, np.asarray(pairs), np.asarray(T0)
