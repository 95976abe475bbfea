"""numpy restatement of mvr_fuse_scene (include/mvreg.h): the fragments mapped by their poses, then Open3D's
VoxelDownSample of the concatenated cloud — overlap_cases.voxel_down_sample_dict's logic (a plain dict of lists, sums
in input order) extended with point counts, distinct fragments and normals, the rows sorted by voxel key.

`margin` is the smallest distance of any (q - lo) / voxel from an integer: the GPU may contract the transform's
multiply-adds and move q by a few ulp, so only a point closer than about 1e-12 to a voxel face could change voxel.
The GPU cases must keep it above MARGIN (asserted on the host by test_fuse_host.py)."""
import functools

import numpy as np

BITS = 21
MARGIN = 1e-9
SHORT_NORMAL = 1e-6      # a summed normal shorter than this has no direction worth comparing


def transform(xyz, R, t):
    """q_d = R[d][0] x + R[d][1] y + R[d][2] z + t_d, the products summed left to right"""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    return np.stack([R[d, 0] * p[:, 0] + R[d, 1] * p[:, 1] + R[d, 2] * p[:, 2] + t[d] for d in range(3)], 1)


def rotate(nrm, R):
    n = np.asarray(nrm, np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float64)
    return np.stack([R[d, 0] * n[:, 0] + R[d, 1] * n[:, 1] + R[d, 2] * n[:, 2] for d in range(3)], 1)


def fuse(frags, R, t, voxel, member=None, normals=None):
    """frags: list of [n_b,3]; R [B,3,3], t [B,3]; member [B] or None; normals: list of [n_b,3] or None.
    -> dict: xyz [V,3], n_points [V], n_frags [V], normals [V,3] or None, normal_len [V] (length of the summed
    normal), keys [V] (ascending), over_range (bool: the GPU must answer -1), margin"""
    B = len(frags)
    member = np.ones(B, bool) if member is None else np.asarray(member).astype(bool)
    q, fid, nr = [], [], []
    for b in range(B):
        if not member[b]:
            continue
        q.append(transform(frags[b], R[b], t[b]))
        fid.append(np.full(len(q[-1]), b))
        if normals is not None:
            nr.append(rotate(normals[b], R[b]))
    q = np.concatenate(q).reshape(-1, 3) if q else np.zeros((0, 3))
    fid = np.concatenate(fid) if fid else np.zeros(0, int)
    nr = np.concatenate(nr).reshape(-1, 3) if nr else None
    empty = {"xyz": np.zeros((0, 3)), "n_points": np.zeros(0, np.int32), "n_frags": np.zeros(0, np.int32),
             "normals": None if normals is None else np.zeros((0, 3)), "normal_len": np.zeros(0),
             "keys": np.zeros(0, np.uint64), "over_range": False, "margin": np.inf}
    if len(q) == 0:
        return empty
    if not np.isfinite(q).all():
        return dict(empty, over_range=True, margin=0.0)
    lo = q.min(0) - voxel * 0.5
    ref = (q - lo) / voxel
    cell = np.floor(ref)
    margin = float(np.minimum(ref - cell, cell + 1.0 - ref).min())
    if (cell < 0).any() or (cell >= 2.0 ** BITS).any():
        return dict(empty, over_range=True, margin=margin)
    cell = cell.astype(np.int64)
    cells = {}
    for i, c in enumerate(cell.tolist()):
        cells.setdefault((c[0] << (2 * BITS)) | (c[1] << BITS) | c[2], []).append(i)
    keys = sorted(cells)
    xyz, n_points, n_frags, nsum = [], [], [], []
    for k in keys:
        rows = cells[k]                      # in input order: ascending fragment, then ascending row
        s = [0.0, 0.0, 0.0]
        sn = [0.0, 0.0, 0.0]
        for i in rows:
            for d in range(3):
                s[d] += q[i, d]
                if nr is not None:
                    sn[d] += nr[i, d]
        xyz.append([s[d] / len(rows) for d in range(3)])
        n_points.append(len(rows))
        n_frags.append(len(set(fid[rows].tolist())))
        nsum.append(sn)
    out = {"xyz": np.asarray(xyz, np.float64).reshape(-1, 3), "n_points": np.asarray(n_points, np.int32),
           "n_frags": np.asarray(n_frags, np.int32), "keys": np.asarray(keys, np.uint64), "over_range": False,
           "margin": margin, "normals": None, "normal_len": np.zeros(len(keys))}
    if nr is not None:
        nsum = np.asarray(nsum, np.float64).reshape(-1, 3)
        ln = np.sqrt(nsum[:, 0] * nsum[:, 0] + nsum[:, 1] * nsum[:, 1] + nsum[:, 2] * nsum[:, 2])
        zero = (nsum == 0.0).all(1)
        out["normals"] = np.where(zero[:, None], np.array([0.0, 0.0, 1.0]), nsum / np.where(zero, 1.0, ln)[:, None])
        out["normal_len"] = ln
    return out


# ------------------------------------------------------------------------------------------- the GPU test's cases
SCENE_VIEW = (3.0, 3.0, 1.5)      # inside the synthetic room, off every plane the four fragments see


def scene_viewpoints(poses):
    """SCENE_VIEW in every fragment's own frame, R^T (W - t): one viewpoint for the whole scene, so that the
    fragments orient a shared surface alike (per-fragment viewpoints such as the fragments' means lie on the surface
    they see, and opposite normals of two fragments then cancel exactly)"""
    poses = np.asarray(poses, np.float64)
    return np.asarray([M[:3, :3].T @ (np.asarray(SCENE_VIEW) - M[:3, 3]) for M in poses])


RUN_SIZES = (1, 255, 256, 257, 4095, 4096, 4097)      # around a workgroup and around the sort's 4096-key tile
V_SMALL = 0.05


def spread_points(n, seed):
    """n points, each in a voxel of its own (a shuffled lattice of pitch 2 voxels with a jitter of 0.4 voxels, so that
    whichever point anchors the grid no two share a voxel; negative coordinates included)"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    p = (g - side // 2) * (2 * V_SMALL) + rng.uniform(0.3, 0.7, (n, 3)) * V_SMALL
    return p[rng.permutation(n)]


def clump_points(n, seed):
    """n points inside one voxel, away from its faces"""
    rng = np.random.default_rng(seed)
    return np.array([-0.3, 0.2, 0.7]) + rng.uniform(0.3, 0.7, (n, 3)) * V_SMALL


def _posed(frags, seed):
    """random rigid poses and unit normals for a list of fragments"""
    rng = np.random.default_rng(seed)
    R, t, nrm = [], [], []
    for f in frags:
        A = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        R.append(A * np.sign(np.linalg.det(A)))
        t.append(rng.normal(0, 0.5, 3))
        v = rng.standard_normal((len(f), 3))
        nrm.append(v / np.linalg.norm(v, axis=1, keepdims=True))
    return np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3), nrm


@functools.lru_cache(maxsize=None)
def size_cases():
    """{name: (frags, R, t, normals)}: every run size as one fragment of separate voxels and as one clump, under
    identity poses (the GPU must then match bit for bit)"""
    out = {}
    for n in RUN_SIZES:
        for kind, make in (("spread", spread_points), ("clump", clump_points)):
            f = [make(n, 100 + n)]
            _, _, nrm = _posed(f, 200 + n)
            out["%s_%d" % (kind, n)] = (f, np.eye(3)[None], np.zeros((1, 3)), nrm)
    return out


@functools.lru_cache(maxsize=None)
def ragged_case():
    """seven fragments, empty ones first, in the middle and last, under random poses; fragment 5 holds
    fragment 1's scene points, each moved by up to a tenth of a voxel, in its own frame (R_5^T (X - t_5)), so the two
    fragments share most of their voxels -> (frags, R, t, normals)"""
    rng = np.random.default_rng(11)
    sizes = (0, 300, 0, 1, 700, 300, 0)
    frags = [rng.uniform(-1.0, 1.0, (n, 3)) for n in sizes]
    R, t, nrm = _posed(frags, 12)
    scene = transform(frags[1], R[1], t[1]) + 0.1 * V_SMALL * rng.uniform(-1, 1, (300, 3))
    frags[5] = (scene - t[5]) @ R[5]          # R^T (scene - t)
    return frags, R, t, nrm


@functools.lru_cache(maxsize=None)
def three_fragment_run_case():
    """four fragments under identity poses and negative coordinates.  Fragment 1's second point, 3.5 voxels below c
    on every axis, is the scene's minimum, so the voxel faces lie at c + k voxel and the voxel [c, c + voxel) has the
    index (4, 4, 4): fragments 0 (two points), 1 (one) and 3 (two) fall into it, a run of five that spans three
    fragments; fragment 2 lies elsewhere -> (frags, R, t, normals)"""
    v = V_SMALL
    c = np.array([-2.0, -3.0, -1.0])
    f0 = np.array([[0.2, 0.3, 0.4], [0.6, 0.5, 0.3], [5.2, 0.3, 0.4]]) * v + c
    f1 = np.array([[0.7, 0.2, 0.6], [-3.5, -3.5, -3.5]]) * v + c
    f2 = np.array([[9.5, 9.5, 9.5]]) * v + c
    f3 = np.array([[0.4, 0.8, 0.2], [0.3, 0.3, 0.3], [-2.6, 0.3, 0.7]]) * v + c
    frags = [f0, f1, f2, f3]
    up = [np.tile([0.0, 0.0, 1.0], (len(f), 1)) for f in frags]
    return frags, np.tile(np.eye(3), (4, 1, 1)), np.zeros((4, 3)), up


def far_case():
    """two fragments, the second posed 2^21 voxels away along y: the index leaves the key -> (frags, R, t)"""
    frags = [clump_points(5, 1), clump_points(5, 2)]
    t = np.zeros((2, 3))
    t[1, 1] = (2.0 ** BITS) * V_SMALL
    return frags, np.tile(np.eye(3), (2, 1, 1)), t
