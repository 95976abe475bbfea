"""numpy restatement, in fp64, of the FPFH descriptors (csrc/fpfh.hip mvr_compute_fpfh) and of the feature matcher
(csrc/feat_match.hip mvr_feat_match), and their test cases.

Open3D and PCL are absent, so parity is pinned to the semantics stated here (include/mvreg.h).  The
neighbour search is sklearn's kd-tree followed by the kernel's own distance expression.

    neighbours of i: the points j != i of its fragment with sqrt(ex*ex + ey*ey + ez*ez) < radius (strict); k_i of them
    pair feature:    e = x_j - x_i, d = |e|, a1 = n_i.e/d, a2 = n_j.e/d; if |a1| < |a2|: (n_a, n_b, e, f2) =
                     (n_j, n_i, -e, -a2) else (n_i, n_j, e, a1); v = (e x n_a)/|e x n_a|, w = n_a x v,
                     f0 = atan2(w.n_b, n_a.n_b), f1 = v.n_b; d == 0 or |e x n_a| == 0: counted in k_i, not binned
    bins:            floor(11 (f0 + pi)/(2 pi)) | 11 + floor(11 (f1 + 1)/2) | 22 + floor(11 (f2 + 1)/2), each clamped
    spfh_i:          100 count_i / k_i (zeros for k_i = 0)
    fpfh_i:          acc = sum_j spfh_j / d_ij^2 over d > 0; each group of 11 with a positive sum scaled to 100;
                     fpfh_i = acc + spfh_i

A histogram is a step function of the features, so two computations can only be compared where no feature sits on a
step.  Every point therefore carries an `unsafe` flag:
    SPFH: a binned feature lies within EDGE (1e-9, in bin units) of an interior bin edge 1..10 (the clamped ends 0 and
          11 are no discontinuities), or ||a1| - |a2|| < EDGE and the two role assignments give different bins (where
          they give the same bins, as everywhere on a plane, the tie is harmless);
    FPFH: the point or any of its neighbours is unsafe for SPFH.
"""
import functools

import numpy as np

import icp_oracle as O
import icp_plane_oracle as PO

EDGE = 1e-9
BINS = 33


def _features(ni, nj, e, d, swap):
    """the three features in bin units [n,3] and the mask of pairs that are binned, for a given role assignment"""
    na = np.where(swap[:, None], nj, ni)
    nb = np.where(swap[:, None], ni, nj)
    a1, a2 = np.einsum("ij,ij->i", ni, e) / d, np.einsum("ij,ij->i", nj, e) / d
    f2 = np.where(swap, -a2, a1)
    es = np.where(swap[:, None], -e, e)
    v = np.cross(es, na)
    vl = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    ok = vl > 0
    v = v / np.where(ok, vl, 1.0)[:, None]
    w = np.cross(na, v)
    f0 = np.arctan2(np.einsum("ij,ij->i", w, nb), np.einsum("ij,ij->i", na, nb))
    f1 = np.einsum("ij,ij->i", v, nb)
    x = np.stack([11.0 * (f0 + np.pi) / (2.0 * np.pi), 11.0 * (f1 + 1.0) / 2.0, 11.0 * (f2 + 1.0) / 2.0], 1)
    return x, ok


def _bins(x):
    return np.clip(np.floor(x), 0, 10).astype(np.int64)


def _near_edge(x):
    """a feature within EDGE of an interior bin edge"""
    k = np.round(x)
    return (np.abs(x - k) < EDGE) & (k >= 1) & (k <= 10)


def fpfh(pts, normals, radius):
    """One fragment.  -> dict(spfh [n,33], fpfh [n,33] fp64, k [n], unsafe_spfh [n], unsafe_fpfh [n])"""
    from sklearn.neighbors import NearestNeighbors
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    normals = np.asarray(normals, np.float64).reshape(-1, 3)
    n = len(pts)
    out = {"spfh": np.zeros((n, BINS)), "fpfh": np.zeros((n, BINS)), "k": np.zeros(n, np.int64),
           "unsafe_spfh": np.zeros(n, bool), "unsafe_fpfh": np.zeros(n, bool)}
    if n == 0:
        return out
    cand = NearestNeighbors(algorithm="kd_tree").fit(pts).radius_neighbors(pts, 1.001 * radius, return_distance=False)
    nbrs, dist2 = [], []
    for i in range(n):
        j = np.sort(cand[i][cand[i] != i])
        e = pts[j] - pts[i]
        d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
        d = np.sqrt(d2)
        near = d < radius
        j, e, d, d2 = j[near], e[near], d[near], d2[near]
        nbrs.append(j)
        dist2.append(d2)
        out["k"][i] = len(j)
        pos = d > 0
        j, e, d = j[pos], e[pos], d[pos]
        if len(j) == 0:
            continue
        ni, nj = np.tile(normals[i], (len(j), 1)), normals[j]
        a1, a2 = np.einsum("ij,ij->i", ni, e) / d, np.einsum("ij,ij->i", nj, e) / d
        swap = np.abs(a1) < np.abs(a2)
        x, ok = _features(ni, nj, e, d, swap)
        b = _bins(x)
        count = np.zeros(BINS, np.int64)
        for g in range(3):
            count += np.bincount(11 * g + b[ok, g], minlength=BINS)
        out["spfh"][i] = 100.0 * count / out["k"][i]
        unsafe = bool(_near_edge(x[ok]).any())
        tie = np.abs(np.abs(a1) - np.abs(a2)) < EDGE
        if tie.any():
            xo, oko = _features(ni[tie], nj[tie], e[tie], d[tie], ~swap[tie])
            differ = (oko != ok[tie]) | (_bins(xo) != b[tie]).any(1) | _near_edge(xo).any(1)
            unsafe = unsafe or bool(differ.any())
        out["unsafe_spfh"][i] = unsafe
    for i in range(n):
        j, d2 = nbrs[i], dist2[i]
        pos = d2 > 0
        acc = (out["spfh"][j[pos]] / d2[pos, None]).sum(0) if pos.any() else np.zeros(BINS)
        for g in range(3):
            s = acc[11 * g:11 * g + 11].sum()
            if s > 0:
                acc[11 * g:11 * g + 11] *= 100.0 / s
        out["fpfh"][i] = acc + out["spfh"][i]
        out["unsafe_fpfh"][i] = out["unsafe_spfh"][i] or bool(out["unsafe_spfh"][j].any())
    return out


def fpfh_batch(frags, normals, radius):
    """-> a list of fpfh() dicts, one per fragment"""
    return [fpfh(f, m, radius) for f, m in zip(frags, normals)]


def ulps32(got, want64):
    """|got - fp32(want64)| in units of the fp32 ulp of fp32(want64) (the ulp of the smallest normal for 0)"""
    w = np.asarray(want64, np.float64).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(w), np.finfo(np.float32).tiny)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - w.astype(np.float64)) / ulp


def nearest_feature(Fq, Ft):
    """fp64 distance of every query row to its nearest target row -> (min dist2 [nq], a row that attains it [nq]);
    (inf, -1) for an empty target.  The row is found on |a|^2 + |b|^2 - 2 a.b (rounding about 1e-16 of the squared
    norms, 1e-11 for FPFH rows) and its distance then taken as sum (a - b)^2: the minimum to that rounding, far below
    the matcher's fp32 bound."""
    Fq, Ft = np.asarray(Fq, np.float64), np.asarray(Ft, np.float64)
    if len(Ft) == 0:
        return np.full(len(Fq), np.inf), np.full(len(Fq), -1, np.int64)
    d = (Fq * Fq).sum(1)[:, None] + (Ft * Ft).sum(1)[None, :] - 2.0 * Fq @ Ft.T
    arg = d.argmin(1)
    return ((Fq - Ft[arg]) ** 2).sum(1), arg


# --------------------------------------------------------------------------------------------------- the test cases
SCENE_RADII = (0.075, 0.05)
SCENE_FRAGS = (0, 1)
CAP_SPFH, CAP_FPFH = 0.01, 0.06       # the largest shares of a scene fragment's rows a comparison may leave out
SMALL_R_INDEX = 0.1
SMALL_RADII = (0.1, 0.04)
SMALL_SIZES = O.SMALL_SIZES           # 0, 1, 2, 3, 63, 64, 65, 1025


@functools.lru_cache(maxsize=None)
def scene_case(radius=0.075):
    """fragments 0 and 1 of the scene's centroids (the oracle's own row order), their normals over 0.075 oriented to
    the fragment's mean, and the oracle's FPFH at `radius` -> (frags, normals, viewpoints, results)"""
    frags = [O.scene4_centroids()[b] for b in SCENE_FRAGS]
    vps = [f.mean(0) for f in frags]
    normals = [PO.estimate_normals(f, PO.NORMAL_RADIUS, v)["normals"] for f, v in zip(frags, vps)]
    return frags, normals, vps, fpfh_batch(frags, normals, radius)


def small_case(seed=0):
    """Fragments of SMALL_SIZES uniformly random points for an index of cell SMALL_R_INDEX, straddling negative
    coordinates, a third of each on cell faces (the construction of icp_oracle.small_case's target), with random unit
    normals; the last two rows of the 65-point fragment coincide exactly (d == 0).  The boxes shrink with the size so
    that every fragment of two or more points has neighbours.  No row may be unsafe at either of SMALL_RADII
    (test_fpfh_host.py checks it); seed 0 is the first that leaves none.  -> (frags, normals)"""
    rng = np.random.default_rng(seed)
    frags, normals = [], []
    for n in SMALL_SIZES:
        half = 0.45 if n > 100 else 0.12 if n > 3 else 0.03
        p = rng.uniform(-half, half, (n, 3))
        m = n // 3
        p[:m] = np.round(p[:m] / SMALL_R_INDEX) * SMALL_R_INDEX + \
            rng.uniform(-0.4, 0.4, (m, 3)) * SMALL_R_INDEX * (rng.random((m, 3)) < 0.5)
        if n == 65:
            p[-1] = p[-2]
        v = rng.standard_normal((n, 3))
        frags.append(p)
        normals.append(v / np.linalg.norm(v, axis=1, keepdims=True))
    return frags, normals
