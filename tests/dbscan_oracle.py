"""numpy restatement of mvr_cluster_dbscan from its contract in include/mvreg.h (not from the kernels), and the cases
tests/test_dbscan_host.py and tests/test_gpu_dbscan.py share.

dbscan is Open3D's sequential cluster_dbscan loop, literally, per fragment: the points are taken in row order as seeds,
a seed with fewer than min_points neighbours is marked noise, any other opens the next cluster and grows it through a
queue; a point marked noise that the queue reaches becomes a border point of that cluster, a point that already has a
cluster keeps it.  The neighbours come from an O(n^2) matrix of sqrt(ex*ex + ey*ey + ez*ez) < eps (strict; the point
itself and its duplicates are among them), every operation rounded on its own.  It shares nothing with the GPU's
union-find."""
import collections
import functools

import numpy as np

import knn_oracle as K


def _within(X, eps):
    """bool [n,n]: row i marks the points closer than eps to point i (strict), in blocks of rows"""
    n = len(X)
    A = np.zeros((n, n), bool)
    for s in range(0, n, 512):
        e = X[None, :, :] - X[s:s + 512, None, :]
        A[s:s + 512] = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) < eps
    return A


def _sequential(X, eps, min_points):
    """Open3D's loop on one cloud -> (labels [n] with -1 for noise, core bool [n])"""
    n = len(X)
    A = _within(X, eps)
    nbrs = [np.flatnonzero(A[i]) for i in range(n)]
    UNSEEN, NOISE = -2, -1
    lab = np.full(n, UNSEEN, np.int64)
    cluster = 0
    for i in range(n):
        if lab[i] != UNSEEN:
            continue
        if len(nbrs[i]) < min_points:
            lab[i] = NOISE
            continue
        lab[i] = cluster
        queue = collections.deque(nbrs[i].tolist())
        visited = set(nbrs[i].tolist())
        visited.add(i)
        while queue:
            nb = queue.popleft()
            if lab[nb] == NOISE:
                lab[nb] = cluster          # reached from a core point: a border point of this cluster
            if lab[nb] != UNSEEN:
                continue
            lab[nb] = cluster
            if len(nbrs[nb]) >= min_points:
                for t in nbrs[nb].tolist():
                    if t not in visited:
                        visited.add(t)
                        queue.append(t)
        cluster += 1
    return lab, A.sum(1) >= min_points


def dbscan(xyz, off, eps, min_points):
    """-> dict labels int32 [M] (a cluster's number within its fragment, -1 noise), n_clusters int64 [B], sizes int32
    [M] (sizes[off[b] + c]: the points labelled c in fragment b, 0 beyond the fragment's clusters), core bool [M]"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    M, B = len(xyz), len(off) - 1
    labels = np.full(M, -1, np.int32)
    sizes = np.zeros(M, np.int32)
    core = np.zeros(M, bool)
    n_clusters = np.zeros(B, np.int64)
    for b in range(B):
        o0, o1 = int(off[b]), int(off[b + 1])
        if o1 == o0:
            continue
        lab, c = _sequential(xyz[o0:o1], eps, min_points)
        labels[o0:o1], core[o0:o1] = lab, c
        n_clusters[b] = lab.max() + 1
        count = np.bincount(lab[lab >= 0], minlength=o1 - o0)
        sizes[o0:o1] = count[:o1 - o0]
    return {"labels": labels, "n_clusters": n_clusters, "sizes": sizes, "core": core}


def margin(xyz, off, eps):
    """the smallest |d - eps| / eps over all pairs of a fragment (how far any decision is from flipping under another
    rounding of d); +inf without points"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = np.inf
    for b in range(len(off) - 1):
        X = xyz[int(off[b]):int(off[b + 1])]
        for s in range(0, len(X), 512):
            e = X[None, :, :] - X[s:s + 512, None, :]
            d = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
            out = min(out, float((np.abs(d - eps) / eps).min()))
    return out


def multi_cluster_borders(xyz, off, eps, res):
    """the border rows (labelled, not core) whose core neighbours lie in more than one cluster -> (borders, of them
    with several clusters)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    borders = several = 0
    for b in range(len(off) - 1):
        o0, o1 = int(off[b]), int(off[b + 1])
        if o1 == o0:
            continue
        A = _within(xyz[o0:o1], eps)
        lab, core = res["labels"][o0:o1], res["core"][o0:o1]
        for i in np.flatnonzero(~core & (lab >= 0)):
            borders += 1
            several += len(set(lab[np.flatnonzero(A[i] & core)].tolist())) > 1
    return borders, several


def cluster_keep(res, off, min_size=None, largest=False):
    """FragmentOverlap.cluster_keep restated: bool [M]"""
    labels, sizes = res["labels"], res["sizes"]
    keep = np.zeros(len(labels), bool)
    for b in range(len(off) - 1):
        o0, o1 = int(off[b]), int(off[b + 1])
        if o1 == o0 or res["n_clusters"][b] == 0:
            continue
        lab, size = labels[o0:o1], sizes[o0:o1]
        if largest:
            keep[o0:o1] = lab == int(np.argmax(size))            # argmax: the first of equal sizes
        else:
            keep[o0:o1] = (lab >= 0) & (size[np.maximum(lab, 0)] >= min_size)
    return keep


# --------------------------------------------------------------------------------------------------------------- cases
# every case: (fragments, the index's cell, eps, min_points)
def clouds_case():
    A, B = K.clouds()[:2]
    return [A, B], K.R_CELL, 0.05, 8


@functools.lru_cache(maxsize=None)
def _blobs():
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 0.11 - 0.2
    x = np.concatenate([c + rng.normal(0, 0.02, (50, 3)) for c in g])
    return x[rng.permutation(len(x))]


def blobs_case():
    """48 Gaussian blobs of 50 points, sigma 0.02, on a 4 x 4 x 3 grid of pitch 0.11: neighbouring blobs touch, so
    some merge and border points lie between clusters"""
    return [_blobs()], K.R_CELL, 0.03, 6


@functools.lru_cache(maxsize=None)
def _helices():
    t = np.arange(3000) * 0.03

    def helix(phase):
        return np.stack([0.5 * np.cos(t / 0.5 + phase), 0.5 * np.sin(t / 0.5 + phase), 0.06 * t], 1)
    x = np.concatenate([helix(0.0), helix(np.pi)])
    return x[np.random.default_rng(9).permutation(len(x))] - np.array([0.2, 0.3, 2.0])


def helices_case():
    """two interleaved helices of 3000 points, 0.03 apart along the curve, rows shuffled: two chains of 3000 edges over
    many cells and workgroups"""
    return [_helices()], 0.075, 0.05, 3


def ties_case():
    frags, r = K.ties_case()
    return frags, r, 0.04, 7


RAGGED_EPS = 0.06


def ragged_case():
    return K.ragged_case(), K.R_CELL, RAGGED_EPS, 5


CASES = {"clouds": clouds_case, "blobs": blobs_case, "helices": helices_case, "ties": ties_case,
         "ragged": ragged_case}


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """(xyz [M,3], off [B+1], the oracle's dict) of a case, computed once"""
    frags, _, eps, min_points = CASES[name]()
    xyz, off = K.stack(frags), K.offsets(frags)
    return xyz, off, dbscan(xyz, off, eps, min_points)


# the scene of knn_oracle.scene_case with a blob planted in each fragment: a piece of another object in front of the
# sensor.  BLOB_POINTS raw points of sigma BLOB_SIGMA around a centre BLOB_OFF off the surface.  register_scene
# clusters the 0.025 m voxel centroids: 150 points of sigma 12 mm leave 18 to 24 centroids inside one ball of 0.075, so
# the radius filter at its defaults (more than 16 neighbours) keeps them (40 points of sigma 5 mm would leave 3 to 5
# centroids, which that filter removes by itself).  The scene's own surfaces have detached pieces of 38 and more
# centroids: min_size 30 lies between the two.
BLOB_POINTS, BLOB_SIGMA, BLOB_OFF = 150, 0.012, 0.3
SCENE_SPEC = {"method": "cluster", "min_points": 10, "min_size": 30, "eps": None}


@functools.lru_cache(maxsize=None)
def scene_blob_case():
    """(raw float32 fragments with the blob appended to each, the blobs as float32)"""
    rng = np.random.default_rng(13)
    frags, blobs = [], []
    for f in K.scene_case()[0]:
        f64 = np.asarray(f, np.float64)
        lo, hi = f64.min(0), f64.max(0)
        centre = None
        for _ in range(2000):   # bounded: a place BLOB_OFF (+- 10 %) from the nearest point of the fragment
            c = rng.uniform(lo, hi)
            d = np.sqrt(((f64 - c) ** 2).sum(1)).min()
            if 0.9 * BLOB_OFF < d < 1.1 * BLOB_OFF:
                centre = c
                break
        assert centre is not None
        blob = (centre + rng.normal(0.0, BLOB_SIGMA, (BLOB_POINTS, 3))).astype(np.float32)
        frags.append(np.concatenate([np.asarray(f, np.float32), blob]))
        blobs.append(blob)
    return frags, blobs
