"""Crafted inputs of the overlap gate (csrc/overlap.hip, csrc/rindex.hpp) at ragged and boundary shapes, shared by
tests/test_overlap_host.py (which pins oracle/overlap.py on them against brute force, on the CPU) and
tests/test_gpu_overlap_edges.py (which pins the kernels on them against that oracle).  Not a test module.

Every case is small (at most 5,000 points in a fragment, at most 3,000 where pairs are counted) and built from fixed
seeds, so both test modules see the same arrays."""
import functools

import numpy as np

V = 0.025                      # the benchmark's voxel size
R = 0.05                       # the '3DMatch' radius
KEY_FIELD = 1 << 16            # values of a voxel / cell coordinate field of pack_key (csrc/rindex.hpp)


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rigid(axis, angle, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(axis, angle), t
    return T


# ------------------------------------------------------------------------------------------- voxel centroids
def _lattice(base, steps, count):
    """count^3 points base + m * steps, m in [0, count)^3 (fp64 arithmetic; exact for the dyadic cases)."""
    m = np.stack(np.meshgrid(*[np.arange(count, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.asarray(base, np.float64) + m * steps


def _face_fragments():
    """Multiples of 2^-6: with v = 2^-5, p - min takes every value (k + 0.5) v (odd multiples) and k v (even ones), so
    every second lattice plane lies exactly on a voxel face and (p - (min - v/2)) / v is exact.  One fragment wholly at
    negative coordinates, one straddling zero, one positive.  All values are exact in fp32."""
    q = 2.0 ** -6
    return [_lattice([-3.0 - 5 * q, -2.0 - q, -7.0], q, 8).astype(np.float32),
            _lattice([-4 * q, -3 * q, -5 * q], q, 8).astype(np.float32),
            _lattice([1.0 + 3 * q, 2 * q, 64.0 + q], q, 8).astype(np.float32)]


def _sum_order_fragment():
    """5,000 points of one voxel whose magnitudes span 40 bits, so the fp64 sum is inexact and depends on the order
    (test_overlap_host.py checks that it does).  The first point is the minimum (0), the rest lie in [0, 0.4 v]."""
    r = np.random.default_rng(41)
    p = (0.4 * V * 10.0 ** r.uniform(-12.0, 0.0, (5000, 3))).astype(np.float32)
    p[0] = 0.0
    return p


@functools.lru_cache(maxsize=None)
def centroid_cases():
    """name -> (fragments [list of float32 [n,3]], voxel size)."""
    c = {}
    r = np.random.default_rng(11)
    # empty fragments first, in the middle and last; one point; the scan / sort tile edge of 4096
    c["ragged"] = ([r.uniform(0.0, 0.3, (n, 3)).astype(np.float32) + np.float32(b)
                    for b, n in enumerate([0, 1, 4095, 0, 4097, 3, 0])], V)
    for B in (1, 2, 3, 33):       # key_bits(B) = 48 + {1, 1, 2, 6}
        rb = np.random.default_rng(100 + B)
        c["frags%d" % B] = ([rb.uniform(0.0, 0.2, (200, 3)).astype(np.float32) - np.float32(0.37 * b)
                             for b in range(B)], V)
    c["faces_dyadic"] = (_face_fragments(), 2.0 ** -5)
    # the same lattice on an inexact voxel size, plus the fp32 roundings of (k + 0.5) * 0.025 themselves
    c["faces_0.025"] = (_face_fragments() + [((_lattice([0.0, 0.0, 0.0], 1.0, 12) + 0.5) * V).astype(np.float32)], V)
    pt = np.array([0.1234, -5.678, 9.1], np.float32)
    c["identical"] = ([np.tile(pt, (300, 1)), np.tile(-pt, (1, 1))], V)
    c["sum_order"] = ([_sum_order_fragment()], V)
    cloud = r.uniform(0.0, 0.3, (1000, 3))
    c["far_translated"] = ([(cloud + 1000.0).astype(np.float32), (cloud - 1000.0).astype(np.float32),
                            (cloud * [1, -1, 1] + [1000.0, -1000.0, 0.0]).astype(np.float32)], V)
    for axis in range(3):         # two clusters 65,533 voxels apart: the largest index stays below the field's 65,535
        c["under_limit_axis%d" % axis] = ([two_clusters(KEY_FIELD - 1 - 2, axis)], V)
    return c


def two_clusters(voxels_apart, axis, v=V):
    """Two 100-point clusters of 0.4 v extent, `voxels_apart` voxels from each other along `axis` (float32)."""
    r = np.random.default_rng(7 + axis)
    a = r.uniform(0.0, 0.4 * v, (100, 3))
    b = r.uniform(0.0, 0.4 * v, (100, 3))
    b[:, axis] += voxels_apart * v
    return np.concatenate([a, b]).astype(np.float32)


def voxel_down_sample_dict(xyz, voxel):
    """Open3D's VoxelDownSample restated with a plain dict of lists: the second, independent host version."""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return p
    lo = [min(row[d] for row in p.tolist()) - voxel * 0.5 for d in range(3)]
    cells = {}
    for row in p.tolist():
        key = tuple(int(np.floor((row[d] - lo[d]) / voxel)) for d in range(3))
        cells.setdefault(key, []).append(row)
    out = []
    for rows in cells.values():
        s = [0.0, 0.0, 0.0]
        for row in rows:              # in input order
            for d in range(3):
                s[d] += row[d]
        out.append([s[d] / len(rows) for d in range(3)])
    return np.array(out, np.float64).reshape(-1, 3)


def lexsorted(a):
    return a[np.lexsort(a.T[::-1])]


# ------------------------------------------------------------------------------------------- overlap counts
class CountCase(object):
    """fragments, method, voxel size, radius override (None: the method's), pairs [P,2], trans [P,4,4] and
    `expect`: {pair row -> (m01, m10)} known without an oracle."""

    def __init__(self, frags, method, pairs, trans, voxel=V, radius=None, expect=None):
        self.frags, self.method, self.voxel, self.radius = frags, method, voxel, radius
        self.pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        self.trans = np.asarray(trans, np.float64).reshape(-1, 4, 4)
        self.expect = expect or {}
        assert len(self.pairs) == len(self.trans)

    @property
    def r(self):
        return self.radius if self.radius is not None else (3 * self.voxel if self.method == "FCGF" else R)


def _exact_r_case():
    """Fragment 0: the origin.  Fragments 1..18: one query each at +-r, +-nextafter(r, 0), +-nextafter(r, 1) along
    x, y, z.  Identity transforms.  sqrt(fl(x * x)) == |x| in IEEE arithmetic, so only the inner one matches."""
    frags, pairs, expect = [np.zeros((1, 3))], [], {}
    for axis in range(3):
        for sign in (1.0, -1.0):
            for d, hit in ((R, 0), (np.nextafter(R, 0.0), 1), (np.nextafter(R, 1.0), 0)):
                q = np.zeros((1, 3))
                q[0, axis] = sign * d
                expect[len(pairs)] = (hit, hit)
                pairs.append((0, len(frags)))
                frags.append(q)
    return CountCase(frags, "3DMatch", pairs, [np.eye(4)] * len(pairs), expect=expect)


def _corner_case():
    """Query and target on opposite sides of a cell corner (cells differ by (+-1, +-1, +-1)), all eight sign
    patterns, at the origin (cell indices change sign) and at an interior corner; at 0.9997 r (match) and
    1.0004 r (no match).  One point per fragment, so the match can only come through that corner cell."""
    frags, pairs, expect = [], [], {}
    for corner in ([0.0, 0.0, 0.0], [3 * R, -2 * R, 5 * R]):
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    s = np.array([sx, sy, sz], np.float64)
                    for half, hit in ((0.2886, 1), (0.2888, 0)):      # |q - t| = 2 sqrt(3) half r
                        expect[len(pairs)] = (hit, hit)
                        pairs.append((len(frags), len(frags) + 1))
                        frags.append((np.asarray(corner) - s * half * R).reshape(1, 3))
                        frags.append((np.asarray(corner) + s * half * R).reshape(1, 3))
    return CountCase(frags, "3DMatch", pairs, [np.eye(4)] * len(pairs), expect=expect)


def _ragged_case(method):
    """Fragments of [3000, 7, 0, 1, 300] points cut from one world cloud under their own poses; every ordered pair,
    self and reversed pairs included, in one call.  Self pairs (0,0), (1,1), (3,3) carry the identity and (4,4) a
    perturbation; of the rest, a third of the transforms are perturbed and the others are the ground truth."""
    r = np.random.default_rng(23)
    world = r.uniform(0.0, 0.6, (3000, 3))
    sizes = [3000, 7, 0, 1, 300]
    poses = [rigid(r.normal(size=3), r.uniform(0.2, 2.5), r.uniform(-1.0, 1.0, 3)) for _ in sizes]
    frags = []
    for n, P in zip(sizes, poses):
        w = world[r.permutation(len(world))[:n]] + r.normal(0.0, 0.004, (n, 3))
        Pi = np.linalg.inv(P)
        frags.append(w @ Pi[:3, :3].T + Pi[:3, 3])          # world -> fragment frame
    pairs, trans, expect = [], [], {}
    for i in range(len(sizes)):
        for j in range(len(sizes)):
            T = np.linalg.inv(poses[i]) @ poses[j]           # fragment j -> fragment i
            if i == j and i != 4:
                T = np.eye(4)
                if method == "3DMatch":                      # 'FCGF': (voxels, voxels), asserted by the GPU test
                    expect[len(pairs)] = (sizes[i], sizes[i])
            elif i == j or (2 * i + j) % 3 == 0:
                T = T @ rigid(r.normal(size=3), r.uniform(0.0, 0.05), r.normal(0.0, 0.03, 3))
            if sizes[i] == 0 or sizes[j] == 0:
                expect[len(pairs)] = (0, 0)
            pairs.append((i, j))
            trans.append(T)
    return CountCase(frags, method, pairs, trans, expect=expect)


def _alias_case():
    """Fragment 0 centred at x = +2000 m, fragment 1 its partner in another frame, fragment 2 = fragment 0 moved by
    exactly 65536 r along x: its cells carry the keys of fragment 0's cells.  Pairs (0,2) and (2,0) under the identity
    probe aliased, occupied cells and must count nothing."""
    r = np.random.default_rng(29)
    a = r.uniform(0.0, 0.5, (500, 3)) + [2000.0, 0.0, 0.0]
    P = rigid([1.0, 2.0, -1.0], 0.7, [3.0, -1.0, 0.5])       # fragment 1 -> fragment 0
    Pi = np.linalg.inv(P)
    b = (a[r.permutation(500)[:400]] + r.normal(0.0, 0.01, (400, 3))) @ Pi[:3, :3].T + Pi[:3, 3]
    c = a + [KEY_FIELD * R, 0.0, 0.0]
    return CountCase([a, b, c], "3DMatch", [(0, 1), (1, 0), (0, 2), (2, 0)], [P, Pi, np.eye(4), np.eye(4)],
                     expect={2: (0, 0), 3: (0, 0)})


def _hash_load_case():
    """3,000 lattice points 0.025 apart on an index of cell size r = 0.01 (the `radius=` path of lib.icp): every
    point has its own cell, as many occupied cells as points.  The query cloud is the lattice jittered by a normal
    of sigma r / 2 per axis, so about three quarters of it stay within r."""
    r = np.random.default_rng(31)
    rad = 0.01
    lat = (_lattice([0.0031, -0.0917, 0.0453], 0.025, 15)[:3000])
    qry = lat + r.normal(0.0, rad / 2, lat.shape)
    small = rigid([0.3, -1.0, 0.2], 0.002, [0.001, -0.002, 0.0015])
    return CountCase([lat, qry], "3DMatch", [(0, 1), (1, 0), (0, 1)], [np.eye(4), np.eye(4), small], radius=rad)


@functools.lru_cache(maxsize=None)
def count_cases():
    return {"exact_r": _exact_r_case(), "corner_cells": _corner_case(), "ragged_3DMatch": _ragged_case("3DMatch"),
            "ragged_FCGF": _ragged_case("FCGF"), "cell_aliasing": _alias_case(), "hash_load": _hash_load_case()}


def cell_keys(xyz, r):
    """The wrapped cell coordinates of cell_key_kernel: (floor(x / r) + 2^15) mod 2^16 per axis."""
    return (np.floor(np.asarray(xyz, np.float64) / r).astype(np.int64) + (KEY_FIELD >> 1)) % KEY_FIELD


@functools.lru_cache(maxsize=None)
def expected_counts(name):
    """[P,2] counts of a case: the oracle (oracle/overlap.py, sklearn's KD-tree as in the reference) for every pair
    of two non-empty fragments, (0, 0) beside an empty one (the reference raises there; lib/overlap.py states 0).
    Computed once per session and shared."""
    from oracle.overlap import overlap_counts
    case = count_cases()[name]
    out = np.zeros((len(case.pairs), 2), np.int64)
    for k, (i, j) in enumerate(case.pairs):
        if len(case.frags[i]) and len(case.frags[j]):
            out[k] = overlap_counts(case.frags[i], case.frags[j], case.trans[k], case.method, case.voxel,
                                    radius=case.radius)[:2]
    out.setflags(write=False)
    return out
