"""numpy restatement of mvr_knn_self, mvr_statistical_outlier and mvr_radius_count from their contract in
include/mvreg.h (not from the kernels), and the cases tests/test_knn_host.py and tests/test_gpu_knn.py share.

knn_self is a brute force per fragment: d2 = (ex*ex + ey*ey) + ez*ez in fp64 with every operation rounded on its own
(numpy never contracts), a stable sort on d2 whose columns are in row order, so equal distances come lower row first."""
import functools

import numpy as np

R_CELL = 0.075    # the index's cell of the cases on the two clouds: 3 voxels of 0.025
K_STAT = 20
STD_RATIO = 2.0
NB_POINTS = 8
N_PLANTED = 30


def offsets(frags):
    return np.concatenate([[0], np.cumsum([len(f) for f in frags])]).astype(np.int64)


def stack(frags):
    return np.concatenate([np.asarray(f, np.float64).reshape(-1, 3) for f in frags]) if len(frags) else \
        np.zeros((0, 3))


def _d2(X):
    """[n,n] squared distances, row i: the candidates of point i"""
    e = X[None, :, :] - X[:, None, :]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def knn_self(xyz, off, k):
    """-> (idx int32 [M,k], dist2 fp64 [M,k]): global rows, -1 / +inf beyond a fragment's size"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    M = len(xyz)
    idx = np.full((M, k), -1, np.int32)
    dist2 = np.full((M, k), np.inf, np.float64)
    for b in range(len(off) - 1):
        o0, o1 = int(off[b]), int(off[b + 1])
        if o1 == o0:
            continue
        d2 = _d2(xyz[o0:o1])
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]
        kk = order.shape[1]
        idx[o0:o1, :kk] = order + o0
        dist2[o0:o1, :kk] = np.take_along_axis(d2, order, axis=1)
    return idx, dist2


def statistical(dist2, off, k, std_ratio):
    """-> dict keep bool [M], mean_dist [M], threshold [B]; fragments below two points keep them, threshold +inf"""
    dist2 = np.asarray(dist2, np.float64).reshape(-1, k)
    keep = np.ones(len(dist2), bool)
    mean_dist = np.zeros(len(dist2))
    thr = np.full(len(off) - 1, np.inf)
    for b in range(len(off) - 1):
        o0, o1 = int(off[b]), int(off[b + 1])
        n = o1 - o0
        if n == 0:
            continue
        kk = min(k, n)
        m = np.sqrt(dist2[o0:o1, :kk]).sum(1) / kk
        mean_dist[o0:o1] = m
        if n < 2:
            continue
        mu = m.sum() / n
        sd = np.sqrt(((m - mu) ** 2).sum() / (n - 1))
        thr[b] = mu + std_ratio * sd
        keep[o0:o1] = m < thr[b]
    return {"keep": keep, "mean_dist": mean_dist, "threshold": thr}


def radius_count(xyz, off, radius, with_margin=False):
    """count int32 [M]: the points of the same fragment with sqrt(ex*ex + ey*ey + ez*ez) < radius, the point itself
    among them.  with_margin: also the smallest |d - radius| / radius over all pairs (how far any decision is from
    flipping under another rounding of d)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    count = np.zeros(len(xyz), np.int32)
    margin = np.inf
    for b in range(len(off) - 1):
        o0, o1 = int(off[b]), int(off[b + 1])
        if o1 == o0:
            continue
        d = np.sqrt(_d2(xyz[o0:o1]))
        count[o0:o1] = (d < radius).sum(1)
        margin = min(margin, float(np.abs(d - radius).min() / radius))
    return (count, margin) if with_margin else count


def resolving_ring(xyz, off, k, r, rho_max=2):
    """Which stage of the search settles a query, by the rule DESIGN.md 4.21a gives (fragments larger than k): ring
    rho is the first with (k-th distance) <= rho r + face - 1e-9 r, face the distance from the point to the nearest
    face of its own cell; 0 when no ring up to rho_max does, the direct scan.  -> int [M]"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    _, dist2 = knn_self(xyz, off, k)
    kd = np.sqrt(dist2[:, k - 1])
    lo = xyz - np.floor(xyz / r) * r
    face = np.minimum(lo, r - lo).min(1)
    ring = np.zeros(len(xyz), np.int64)
    for rho in range(rho_max, 0, -1):
        ring[kd <= rho * r + face - 1e-9 * r] = rho
    return ring


# --------------------------------------------------------------------------------------------------------------- cases
def surface(n, half, offset, seed):
    """n points of z = 0.15 sin(3 u0) cos(2 u1) + N(0, 0.002) over u ~ U(-half, half)^2, moved by offset"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-half, half, (n, 2))
    z = 0.15 * np.sin(3.0 * u[:, 0]) * np.cos(2.0 * u[:, 1]) + rng.normal(0.0, 0.002, n)
    return np.concatenate([u, z[:, None]], 1) + np.asarray(offset, np.float64)


def planted(points, seed, n=N_PLANTED):
    """n copies of random points moved by +-U(0.1, 0.3) along z"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(points), n)
    shift = rng.choice([-1.0, 1.0], n) * rng.uniform(0.1, 0.3, n)
    out = points[pick].copy()
    out[:, 2] += shift
    return out


@functools.lru_cache(maxsize=None)
def clouds():
    """(fragment A, fragment B, is_planted A, is_planted B): 2000 / 1200 surface points with 30 planted outliers each
    behind them; negative coordinates in every axis"""
    out, flags = [], []
    for n, half, offset, seed in ((2000, 0.4, (0.3, -0.4, 1.2), 1), (1200, 0.3, (-2.0, 0.5, -0.7), 2)):
        s = surface(n, half, offset, seed)
        out.append(np.concatenate([s, planted(s, seed + 10)]))
        flags.append(np.arange(n + N_PLANTED) >= n)
    return out[0], out[1], flags[0], flags[1]


@functools.lru_cache(maxsize=None)
def clouds_knn(k):
    """the oracle on [A, B], computed once per k"""
    A, B = clouds()[:2]
    return knn_self(stack([A, B]), offsets([A, B]), k)


def ragged_case():
    """fragments of 0, 1, 5, 19, 20 and 21 points, each inside a few cells of R_CELL"""
    rng = np.random.default_rng(5)
    return [rng.uniform(-0.1, 0.1, (n, 3)) + rng.normal(0, 1.0, 3) for n in (0, 1, 5, 19, 20, 21)]


def sparse_case():
    """300 points in a 3 m cube: at a cell of 0.05 almost no query finds 8 neighbours within two rings"""
    return [np.random.default_rng(6).uniform(-1.5, 1.5, (300, 3))], 0.05, 8


def isolated_case():
    """cloud A and five points 4 to 6 m from it"""
    A = clouds()[0]
    rng = np.random.default_rng(7)
    d = rng.normal(size=(5, 3))
    far = A.mean(0) + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(4.0, 6.0, (5, 1))
    return [np.concatenate([A, far])]


N_SCENE_PLANTED = 20


def free_points(points, rng, n=N_SCENE_PLANTED):
    """n positions in the box of `points`, each 0.15 to 0.3 m from the nearest of them and more than 0.15 m from each
    other: flying pixels in free space"""
    f = np.asarray(points, np.float64)
    lo, hi = f.min(0), f.max(0)
    out = []
    for _ in range(200):   # bounded; a draw of 64 yields several
        c = rng.uniform(lo, hi, (64, 3))
        d = np.sqrt(((c[:, None, :] - f[None, :, :]) ** 2).sum(2)).min(1)
        for p, dd in zip(c, d):
            if len(out) < n and 0.15 < dd < 0.3 and all(np.linalg.norm(p - q) > 0.15 for q in out):
                out.append(p)
        if len(out) == n:
            break
    assert len(out) == n
    return np.asarray(out)


@functools.lru_cache(maxsize=None)
def scene_case():
    """(raw float32 fragments of icp_oracle.scene4 with 20 flying pixels appended to each, those points per fragment
    as float32)"""
    import icp_oracle as O
    rng = np.random.default_rng(3)
    frags, flying = [], []
    for f in O.scene4()[0]:
        p = free_points(f, rng).astype(np.float32)
        frags.append(np.concatenate([np.asarray(f, np.float32), p]))
        flying.append(p)
    return frags, flying


def ties_case():
    """a 12^3 lattice of spacing 1/32 around the origin (power-of-two fractions: coordinates sit exactly on the faces
    of cells of 3/32 and distances tie exactly) and 50 points stored three times each, rows shuffled -> (frags, r)"""
    g = (np.arange(12) - 6) / 32.0
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(8)
    dup = rng.uniform(-0.2, 0.2, (50, 3))
    pts = np.concatenate([lattice, dup, dup, dup])
    return [pts[rng.permutation(len(pts))]], 0.09375
