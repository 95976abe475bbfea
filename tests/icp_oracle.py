"""numpy restatement of the point-to-point ICP refinement (csrc/icp.hip mvr_icp_refine) and its test cases.

Open3D is absent, so parity is pinned to the loop stated below (include/mvreg.h) and to ground
truth.  The nearest neighbour is exact (sklearn's kd-tree in fp64, the library oracle/overlap.py uses), the solve
np.linalg.svd; the kernel walks a cell hash and solves with a Jacobi SVD.

    eval(T):  q = R x + t per source point, y = the nearest target point, valid iff |q - y| < max_dist (strict);
              n_corr, fitness = n_corr / n_src (0 for n_src = 0), rmse = sqrt(sum d^2 / n_corr) (0 for n_corr = 0)
    state = eval(T0)
    for k in 1..max_iters:
        if state.n_corr < 3: status |= 1; break
        T = argmin sum_valid |R x + t - y|^2          (Kabsch on the original source points, det-corrected)
        new = eval(T)
        converged = |new.fitness - state.fitness| < tol_fitness and |new.rmse - state.rmse| < tol_rmse
        state = new
        if converged: break
    if the loop ran max_iters times without `converged` and (tol_fitness > 0 or tol_rmse > 0): status |= 2
    status 4: a fragment index outside [0, B) or a non-finite T0 -> T = T0, everything else 0, trace all -1.

Two results can only be compared where the discrete choices are not decided by rounding, so every evaluation also
reports its margins: the smallest gap between a valid query's nearest and second-nearest distance, and the smallest
|d - max_dist| over the queries; and every loop its |delta fitness| / |delta rmse| history.
"""
import functools

import numpy as np


def evaluate(src, tgt, T, max_dist):
    """-> dict(n_corr, fitness, rmse, valid [n], idx [n], gap, edge) of eval(T); T 3x4 or 4x4"""
    from sklearn.neighbors import NearestNeighbors
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    n, m = len(src), len(tgt)
    out = {"n_corr": 0, "fitness": 0.0, "rmse": 0.0, "valid": np.zeros(n, bool), "idx": np.zeros(n, np.int64),
           "gap": np.inf, "edge": np.inf}
    if n == 0 or m == 0:
        return out
    q = src @ T[:3, :3].T + T[:3, 3]
    d, idx = NearestNeighbors(n_neighbors=min(2, m), algorithm="kd_tree").fit(tgt).kneighbors(q)
    valid = d[:, 0] < max_dist
    nc = int(valid.sum())
    out.update(n_corr=nc, fitness=nc / n, rmse=float(np.sqrt(np.sum(d[valid, 0] ** 2) / nc)) if nc else 0.0,
               valid=valid, idx=idx[:, 0], edge=float(np.min(np.abs(d[:, 0] - max_dist))))
    if m > 1 and nc:
        out["gap"] = float(np.min(d[valid, 1] - d[valid, 0]))
    return out


def kabsch(x, y):
    """argmin_{R, t} sum |R x_i + t - y_i|^2, R in SO(3) -> 3x4"""
    mx, my = x.mean(0), y.mean(0)
    U, _, Vt = np.linalg.svd((x - mx).T @ (y - my))
    R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    return np.concatenate([R, (my - R @ mx)[:, None]], 1)


def icp(src, tgt, T0, max_dist, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6):
    """One pair.  -> dict(T [3,4], fitness, rmse, n_corr, iters, status, trace [max_iters + 1, 2],
    margins [(gap, edge) per evaluation], deltas [(|d fitness|, |d rmse|) per evaluation after the first])"""
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    T = np.array(np.asarray(T0, np.float64)[:3], np.float64)
    trace = np.full((max_iters + 1, 2), -1.0)
    st = evaluate(src, tgt, T, max_dist)
    trace[0] = st["fitness"], st["rmse"]
    margins, deltas = [(st["gap"], st["edge"])], []
    k, status, converged = 0, 0, False
    while k < max_iters:
        if st["n_corr"] < 3:
            status |= 1
            break
        T = kabsch(src[st["valid"]], tgt[st["idx"][st["valid"]]])
        k += 1
        new = evaluate(src, tgt, T, max_dist)
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
            "status": status, "trace": trace, "margins": margins, "deltas": deltas}


def icp_batch(frags, pairs, T0, max_dist, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6):
    """The batch as mvr_icp_refine sees it: frags a list of [n_b, 3], pairs [P, 2], T0 [P, 3 or 4, 4] -> a list of
    icp() dicts; an invalid pair comes out with status 4"""
    out = []
    for (s, g), T in zip(np.asarray(pairs).reshape(-1, 2), np.asarray(T0, np.float64)):
        if not (0 <= s < len(frags) and 0 <= g < len(frags)) or not np.all(np.isfinite(T[:3])):
            out.append({"T": T[:3].copy(), "fitness": 0.0, "rmse": 0.0, "n_corr": 0, "iters": 0, "status": 4,
                        "trace": np.full((max_iters + 1, 2), -1.0), "margins": [], "deltas": []})
        else:
            out.append(icp(frags[s], frags[g], T, max_dist, max_iters, tol_fitness, tol_rmse))
    return out


def min_margins(results):
    """(smallest gap, smallest edge) over every evaluation of every result"""
    m = [mm for r in results for mm in r["margins"]]
    return (min([g for g, _ in m] + [np.inf]), min([e for _, e in m] + [np.inf]))


# --------------------------------------------------------------------------------------------------- the test cases
def rigid(axis, deg, t):
    """4x4 rotation by deg degrees about `axis`, then translation t"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    M[:3, 3] = t
    return M


def perturb(T, centre, rng, deg, sigma):
    """T followed by a rotation of deg degrees about a random axis through `centre` (a point of the target frame) and
    a translation ~ N(0, sigma^2) per axis"""
    D = rigid(rng.standard_normal(3), deg, np.zeros(3))
    D[:3, 3] = centre - D[:3, :3] @ centre + rng.normal(0, sigma, 3)
    return D @ T


@functools.lru_cache(maxsize=None)
def scene4():
    """(raw float32 fragments, poses) of the 4-fragment synthetic scene"""
    from synth import synth_scene_fragments
    return synth_scene_fragments(n_frag=4, seed=7, n_pts=30000, density=26000.0)


@functools.lru_cache(maxsize=None)
def scene4_centroids():
    """the scene's 0.025 m voxel centroids per fragment (the point sets FragmentOverlap(.., 'FCGF') holds; its rows
    come in another order)"""
    from oracle.overlap import voxel_down_sample
    return [voxel_down_sample(f, 0.025) for f in scene4()[0]]


def gt_transform(poses, i, j):
    """source i -> target j"""
    return np.linalg.inv(poses[j]) @ poses[i]


SIX = [(i, j) for i in range(4) for j in range(i + 1, 4)]
TWELVE = SIX + [(j, i) for i, j in SIX]


def scene4_starts(pairs, frags, deg=4.0, sigma=0.03, seed=0):
    """ground truth of every pair perturbed by deg degrees about the source's image centre and N(0, sigma^2)"""
    poses = scene4()[1]
    rng = np.random.default_rng(seed)
    out = []
    for i, j in pairs:
        T = gt_transform(poses, i, j)
        c = (np.asarray(frags[i], np.float64) @ T[:3, :3].T + T[:3, 3]).mean(0)
        out.append(perturb(T, c, rng, deg, sigma))
    return np.asarray(out)


def pair_case():
    """the icp_pair case on raw points: every eighth point of fragments 0 and 1 (from row 4: of the eight offsets
    three leave a nearest-neighbour gap below 1e-8), the first of the six starts
    -> (src, tgt, T0 4x4, max_dist, max_iters)"""
    raw = scene4()[0]
    return raw[0][4::8], raw[1][4::8], scene4_starts(SIX, scene4_centroids())[0], 0.06, 5


def eval_starts(frags):
    """the 12 ordered pairs' transforms of the evaluation-only case: ground truth for even rows, perturbed for odd.
    (Of the raw fragments' 180,000 perturbed queries a few usually have two neighbours within 1e-8 of each other:
    seed 30 is the first of 12..39 that leaves both margins above it.)"""
    poses = scene4()[1]
    T = np.asarray([gt_transform(poses, i, j) for i, j in TWELVE])
    P = scene4_starts(TWELVE, frags, deg=2.0, sigma=0.02, seed=30)
    T[1::2] = P[1::2]
    return T


def full_copy_case(src, seed=3, n_distract=500):
    """target = the source moved by a known rigid motion plus uniform distractors in its box, shuffled; the start is
    1 degree / 5 mm off.  -> (target, T_true 4x4, T_start 4x4)"""
    rng = np.random.default_rng(seed)
    src = np.asarray(src, np.float64)
    Tt = rigid(rng.standard_normal(3), 37.0, rng.normal(0, 1.0, 3))
    moved = src @ Tt[:3, :3].T + Tt[:3, 3]
    tgt = np.concatenate([moved, rng.uniform(moved.min(0), moved.max(0), (n_distract, 3))])
    tgt = tgt[rng.permutation(len(tgt))]
    D = rigid(rng.standard_normal(3), 1.0, np.zeros(3))
    c = moved.mean(0)
    u = rng.standard_normal(3)
    D[:3, 3] = c - D[:3, :3] @ c + 0.005 * u / np.linalg.norm(u)
    return tgt, Tt, D @ Tt


SMALL_SIZES = (0, 1, 2, 3, 63, 64, 65, 1025)
SMALL_RADIUS, SMALL_MAX_DIST = 0.1, 0.1


def small_case(seed=2):
    """Raw-point fragments for FragmentOverlap(.., '3DMatch', radius=SMALL_RADIUS): fragment 0 a 300-point target
    that straddles negative coordinates, a third of it on cell faces (coordinates that are multiples of the cell
    size); fragments 1.. sources of SMALL_SIZES points (jittered target points, moved by a known motion) and one
    far-away source.  -> (frags, pairs [P,2], T0 [P,4,4])"""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-0.45, 0.45, (300, 3))
    tgt[:100] = np.round(tgt[:100] / SMALL_RADIUS) * SMALL_RADIUS + \
        rng.uniform(-0.4, 0.4, (100, 3)) * SMALL_RADIUS * (rng.random((100, 3)) < 0.5)
    Tt = rigid([1.0, 2.0, -0.5], 25.0, [0.3, -0.2, 0.1])          # source -> target
    Ti = np.linalg.inv(Tt)
    frags, pairs, T0 = [tgt], [], []
    for n in SMALL_SIZES:
        pick = np.arange(n) % 300 if n <= 300 else rng.integers(0, 300, n)
        p = tgt[pick] + rng.normal(0, 0.004, (n, 3))
        frags.append(p @ Ti[:3, :3].T + Ti[:3, 3])
        pairs.append((len(frags) - 1, 0))
        T0.append(perturb(Tt, np.zeros(3), rng, 1.5, 0.004))
    frags.append(tgt[:40] + 100.0)                                   # no correspondence at the start
    pairs.append((len(frags) - 1, 0))
    T0.append(np.eye(4))
    return frags, np.asarray(pairs), np.asarray(T0)
