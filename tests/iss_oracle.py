"""numpy restatement of mvr_iss_saliency and mvr_radius_nms from their contract in include/mvreg.h (not from the
kernels), and the cases tests/test_iss_host.py and tests/test_gpu_iss.py share.

Neighbourhoods are brute force per fragment: the points with sqrt((ex*ex + ey*ey) + ez*ez) < radius in fp64, the point
itself among them.  The covariance is taken about the neighbours' own mean in coordinates relative to the point and
divided by their number; its eigenvalues come from np.linalg.eigvalsh.

Two results can only be compared where the decisions are not made by rounding, so every decision reports its margin:
  radius margin   the smallest |d - radius| / radius over all pairs of a fragment (n_nbr and the ball's members);
  saliency        per point with enough neighbours, from the relative distances of l2 / l1, l3 / l2 and l3 / l1 to
                  gamma_21, gamma_32 and min_ratio: a candidate passed all three tests, so its margin is the smallest
                  of the three; a rejected point failed at least one, and the widest failure alone settles it, so its
                  margin is the largest among the failed tests;
  NMS             per point with a positive score and a full enough ball, the relative gap |s_j - s_i| / s_i to the
                  competing score that decides: the largest score among the other points of the ball.  Above s_i by
                  the margin it suppresses i whatever the rest does, below s_i by the margin so is every other, and no
                  third case exists, so this gap is exactly how far the decision is from flipping (0 on an exact tie
                  with the largest, where the row order decides; +inf without a competitor).  `nearest` is the gap to
                  the closest score of the ball instead, decisive or not: never larger, so a stricter exclusion; it is
                  small wherever two close points share their neighbour set, also below a clear maximum."""
import functools

import numpy as np

import icp_oracle as O
import icp_plane_oracle as PO
import knn_oracle as K

GAMMA_21 = GAMMA_32 = 0.975
MIN_NEIGHBORS = 5
MIN_RATIO = 1e-6
CHUNK = 256


def _ball(X, rows, radius):
    """(member bool [len(rows), n], e [len(rows), n, 3], smallest |d - radius| / radius) for the points `rows` of X"""
    e = X[None, :, :] - X[rows, None, :]
    d = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    return d < radius, e, float(np.abs(d - radius).min() / radius)


def saliency(xyz, off, radius, gamma_21=GAMMA_21, gamma_32=GAMMA_32, min_ratio=MIN_RATIO,
             min_neighbors=MIN_NEIGHBORS):
    """-> dict saliency fp64 [M] (l3 of a candidate, -1.0 otherwise), n_nbr int32 [M], eig fp64 [M,3] (l1 >= l2 >= l3;
    0 where n_nbr < min_neighbors), candidate bool [M], margin fp64 [M] (+inf where n_nbr < min_neighbors: that
    decision is exact), radius_margin"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    M = len(xyz)
    sal, n_nbr, eig = np.full(M, -1.0), np.zeros(M, np.int32), np.zeros((M, 3))
    margin, rmargin = np.full(M, np.inf), np.inf
    for b in range(len(off) - 1):
        o0, o1 = int(off[b]), int(off[b + 1])
        X = xyz[o0:o1]
        for c0 in range(0, o1 - o0, CHUNK):
            rows = np.arange(c0, min(c0 + CHUNK, o1 - o0))
            W, e, rm = _ball(X, rows, radius)
            rmargin = min(rmargin, rm)
            n = W.sum(1)
            Wf = W.astype(np.float64)
            mean = (Wf[..., None] * e).sum(1) / n[:, None]
            dev = (e - mean[:, None, :]) * Wf[..., None]
            C = np.einsum("ija,ijb->iab", dev, dev) / n[:, None, None]
            n_nbr[o0 + rows] = n
            eig[o0 + rows] = np.linalg.eigvalsh(C)[:, ::-1]
    enough = n_nbr >= min_neighbors
    eig[~enough] = 0.0
    l1, l2, l3 = eig[:, 0], eig[:, 1], eig[:, 2]
    tests = np.stack([l2 < gamma_21 * l1, l3 < gamma_32 * l2, l3 > min_ratio * l1], 1)
    cand = enough & tests.all(1)
    sal[cand] = l3[cand]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.stack([np.abs(l2 / l1 - gamma_21) / gamma_21, np.abs(l3 / l2 - gamma_32) / gamma_32,
                        np.abs(l3 / l1 - min_ratio) / min_ratio if min_ratio > 0 else np.full(M, np.inf)], 1)
    rel = np.where(np.isnan(rel), 0.0, rel)          # 0 / 0: a degenerate neighbourhood, no margin claimed
    m_cand = rel.min(1)
    m_rej = np.where(~tests, rel, -np.inf).max(1)
    margin[enough] = np.where(cand, m_cand, m_rej)[enough]
    return {"saliency": sal, "n_nbr": n_nbr, "eig": eig, "candidate": cand, "margin": margin,
            "radius_margin": rmargin}


def nms(xyz, off, radius, min_neighbors, score):
    """-> dict keep bool [M], decided bool [M] (score > 0 and at least min_neighbors points in the ball: the points
    whose competitors matter), margin and nearest fp64 [M] (+inf where not decided or without a competitor),
    radius_margin"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    score = np.asarray(score, np.float64).reshape(-1)
    M = len(xyz)
    keep, decided, margin, rmargin = np.zeros(M, bool), np.zeros(M, bool), np.full(M, np.inf), np.inf
    nearest = np.full(M, np.inf)
    for b in range(len(off) - 1):
        o0, o1 = int(off[b]), int(off[b + 1])
        X, s = xyz[o0:o1], score[o0:o1]
        for c0 in range(0, o1 - o0, CHUNK):
            rows = np.arange(c0, min(c0 + CHUNK, o1 - o0))
            W, _, rm = _ball(X, rows, radius)
            rmargin = min(rmargin, rm)
            n = W.sum(1)
            other = W & (np.arange(o1 - o0)[None, :] != rows[:, None])
            si = s[rows][:, None]
            with np.errstate(invalid="ignore", divide="ignore"):
                beats = other & ((s[None, :] > si) | ((s[None, :] == si) & (np.arange(o1 - o0)[None, :] < rows[:, None])))
                dec = (s[rows] > 0) & (n >= min_neighbors)
                rival = other & ~np.isnan(s)[None, :]
                top = np.where(rival, s[None, :], -np.inf).max(1)
                gap = np.where(rival.any(1), np.abs(top - s[rows]), np.inf) / s[rows]
                near = np.where(rival, np.abs(s[None, :] - si), np.inf).min(1) / s[rows]
            keep[o0 + rows] = dec & ~beats.any(1)
            decided[o0 + rows] = dec
            margin[o0 + rows] = np.where(dec, gap, np.inf)
            nearest[o0 + rows] = np.where(dec, near, np.inf)
    return {"keep": keep, "decided": decided, "margin": margin, "nearest": nearest, "radius_margin": rmargin}


def iss(xyz, off, salient_radius, non_max_radius, gamma_21=GAMMA_21, gamma_32=GAMMA_32, min_ratio=MIN_RATIO,
        min_neighbors=MIN_NEIGHBORS):
    """the detector end to end -> (saliency dict, nms dict of its saliency)"""
    s = saliency(xyz, off, salient_radius, gamma_21, gamma_32, min_ratio, min_neighbors)
    return s, nms(xyz, off, non_max_radius, min_neighbors, s["saliency"])


# --------------------------------------------------------------------------------------------------------------- cases
SMALL_R_INDEX = PO.SMALL_R_INDEX      # 0.1
PLANAR = PO.PLANAR                    # the fragment of the small batch that lies exactly in z = 0

# name -> (fragments, the index's cell, salient radius, non-max radius); the non-max radius is 2/3 of the salient one
# throughout, the ratio of iss_keypoints' defaults (Open3D's 6 : 4)
CASES = ("clouds", "small", "small_075", "small_04")


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "clouds":             # two surfaces with planted outliers, radius 0.05 on the 0.075 index
        return list(K.clouds()[:2]), K.R_CELL, K.R_CELL, 0.05
    small = PO.small_normals_case()  # 0, 1, 2, 3, 63, 64 (planar), 65 and 1025 points around the origin
    if name == "small":
        return small, SMALL_R_INDEX, SMALL_R_INDEX, 2.0 * SMALL_R_INDEX / 3.0
    if name == "small_075":          # radii below the cell: the walk culls cells
        return small, SMALL_R_INDEX, 0.075, 0.05
    if name == "small_04":
        return small, SMALL_R_INDEX, 0.04, 2.0 * 0.04 / 3.0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """(saliency dict, nms dict) of the case, computed once"""
    frags, _, sal_r, nms_r = case(name)
    return iss(K.stack(frags), K.offsets(frags), sal_r, nms_r)


def bump_patch(n=900, seed=11, bump=0.04):
    """a noisy flat patch of 0.6 m with one Gaussian bump of height `bump` at the origin (0: no bump) -> [n,3]"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-0.3, 0.3, (n, 2))
    z = bump * np.exp(-(u ** 2).sum(1) / (2 * 0.03 ** 2)) + rng.normal(0, 1e-9, n)
    return np.concatenate([u, z[:, None]], 1)


def planted_scores(n, seed):
    """scores on a grid of 1/4 (many exact ties, zeros and negatives) with one row in twenty NaN"""
    rng = np.random.default_rng(seed)
    s = np.round(rng.normal(0.5, 1.0, n) * 4.0) / 4.0
    s[rng.random(n) < 0.05] = np.nan
    return s


def ties_scores(pts):
    """a score that depends on the position alone, on a coarse grid: the stored copies of a point tie exactly, and
    so do lattice neighbours"""
    return 1.0 + np.floor(np.asarray(pts)[:, 0] * 16.0) / 8.0 + np.floor(np.asarray(pts)[:, 1] * 16.0) / 64.0


# the registration case of tests/test_gpu_fpfh.py: fragment 0's centroids and their moved, distracted, shuffled copy
COPY_R_INDEX = 0.075
COPY_NON_MAX = 0.035     # chosen on the CPU: test_iss_host.py asserts the keypoint counts it gives
COPY_MIN_KEYPOINTS, COPY_MIN_REPEATED = 50, 25


@functools.lru_cache(maxsize=None)
def copy_case():
    """(source, target, T_true 4x4)"""
    src = O.scene4_centroids()[0]
    tgt, Tt, _ = O.full_copy_case(src)
    return src, tgt, Tt


@functools.lru_cache(maxsize=None)
def copy_oracle():
    src, tgt, _ = copy_case()
    return iss(K.stack([src, tgt]), K.offsets([src, tgt]), COPY_R_INDEX, COPY_NON_MAX)


def repeated(src, tgt, Tt, keep, tol=1e-9):
    """the source keypoints whose moved position is a target keypoint (within tol) -> bool [number of source
    keypoints]"""
    ks, kt = src[keep[:len(src)]], tgt[keep[len(src):]]
    moved = ks @ Tt[:3, :3].T + Tt[:3, 3]
    if len(kt) == 0:
        return np.zeros(len(ks), bool)
    d = np.sqrt(((moved[:, None, :] - kt[None, :, :]) ** 2).sum(2))
    return d.min(1) < tol


def _nearest(A, B):
    return ((A[:, None, :] - B[None, :, :]) ** 2).sum(2).argmin(1)


@functools.lru_cache(maxsize=None)
def copy_matches(match):
    """The mutual matches lib.fpfh.match_keypoints is specified to give on copy_case with the oracle's own normals,
    FPFH descriptors (rounded to fp32, as the library stores them) and keypoints -> (rows int64 [n,2] within the two
    fragments, inlier bool [n]: the moved source point lies within 0.05, the RANSAC distance, of the target point)"""
    import fpfh_oracle as FO
    src, tgt, Tt = copy_case()
    c = src.mean(0)
    F = []
    for pts, vp in ((src, c), (tgt, Tt[:3, :3] @ c + Tt[:3, 3])):
        nrm = PO.estimate_normals(pts, COPY_R_INDEX, vp)["normals"]
        F.append(FO.fpfh(pts, nrm, COPY_R_INDEX)["fpfh"].astype(np.float32).astype(np.float64))
    keep = copy_oracle()[1]["keep"]
    ks, kt = np.flatnonzero(keep[:len(src)]), np.flatnonzero(keep[len(src):])
    if match == "all":
        kt = np.arange(len(tgt))
    st, ts = _nearest(F[0][ks], F[1][kt]), _nearest(F[1][kt], F[0][ks])
    mutual = ts[st] == np.arange(len(ks))
    rows = np.stack([ks[mutual], kt[st[mutual]]], 1)
    moved = src @ Tt[:3, :3].T + Tt[:3, 3]
    return rows, np.linalg.norm(moved[rows[:, 0]] - tgt[rows[:, 1]], axis=1) < 0.05
