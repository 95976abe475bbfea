"""The overlap oracle (oracle/overlap.py) pinned on the crafted inputs of tests/overlap_cases.py, on the CPU, before
tests/test_gpu_overlap_edges.py leans on it: `overlap_counts` (sklearn's KD-tree, as in the reference) against a
brute-force fp64 all-pairs `sqrt(sum(d * d)) < r`, `voxel_down_sample` against a dict-of-lists restatement, and the
properties that make each crafted input exercise what it is meant to."""
import numpy as np
import pytest

import overlap_cases as C
from oracle.overlap import overlap_counts, voxel_down_sample


def _brute(q, t, r):
    """number of rows of q with some row of t at fp64 distance < r (all pairs, in query chunks)."""
    n = 0
    for s in range(0, len(q), 500):
        d = q[s:s + 500, None, :] - t[None, :, :]
        n += int((np.sqrt((d * d).sum(-1)) < r).any(axis=1).sum())
    return n


def _brute_counts(case, k):
    i, j = case.pairs[k]
    pi, pj = np.asarray(case.frags[i], np.float64), np.asarray(case.frags[j], np.float64)
    if case.method == "FCGF":
        pi, pj = voxel_down_sample(pi, case.voxel), voxel_down_sample(pj, case.voxel)
    T = case.trans[k]
    Ti = np.linalg.inv(T)
    pi_t = (Ti[0:3, 0:3] @ pi.T + Ti[0:3, 3].reshape(-1, 1)).T      # the oracle's (= the reference's) mapping
    pj_t = (T[0:3, 0:3] @ pj.T + T[0:3, 3].reshape(-1, 1)).T
    return _brute(pi, pj_t, case.r), _brute(pj, pi_t, case.r)


@pytest.mark.parametrize("name", sorted(C.count_cases()))
def test_overlap_counts_equal_brute_force(name):
    case = C.count_cases()[name]
    assert max(len(f) for f in case.frags) <= 3000
    exp = C.expected_counts(name)
    checked = 0
    for k, (i, j) in enumerate(case.pairs):
        if len(case.frags[i]) == 0 or len(case.frags[j]) == 0:
            assert tuple(exp[k]) == (0, 0)
            continue
        assert tuple(exp[k]) == _brute_counts(case, k), (name, k, i, j)
        checked += 1
    assert checked > 0
    for k, e in case.expect.items():                                # the answers known without any oracle
        assert tuple(exp[k]) == tuple(e), (name, k)


def test_radius_argument_overrides_the_method():
    a = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    b = np.array([[0.03, 0.0, 0.0], [1.2, 0.0, 0.0]])
    assert overlap_counts(a, b, np.eye(4), "3DMatch")[:2] == (1, 1)
    assert overlap_counts(a, b, np.eye(4), "3DMatch", radius=0.01)[:2] == (0, 0)
    assert overlap_counts(a, b, np.eye(4), "3DMatch", radius=0.25)[:2] == (2, 2)
    assert overlap_counts(a, b, np.eye(4), "FCGF", 0.025, radius=0.01)[:2] == (0, 0)


@pytest.mark.parametrize("name", sorted(C.centroid_cases()))
def test_voxel_down_sample_equals_dict_restatement(name):
    frags, v = C.centroid_cases()[name]
    for f in frags:
        a, b = voxel_down_sample(f, v), C.voxel_down_sample_dict(f, v)
        assert a.shape == b.shape
        np.testing.assert_array_equal(C.lexsorted(a), C.lexsorted(b))


# ---------------------------------------------------------------- the crafted inputs do what they are meant to
def test_case_properties_centroids():
    cc = C.centroid_cases()
    assert [len(f) for f in cc["ragged"][0]] == [0, 1, 4095, 0, 4097, 3, 0]
    assert [len(cc["frags%d" % B][0]) for B in (1, 2, 3, 33)] == [1, 2, 3, 33]
    # dyadic lattice: every odd multiple of 2^-6 above the minimum sits exactly on a voxel face
    frags, v = cc["faces_dyadic"]
    assert (frags[0] < 0).all() and (frags[1] < 0).any() and (frags[1] > 0).any()
    for f in frags:
        ref = (f.astype(np.float64) - (f.min(0).astype(np.float64) - v / 2)) / v
        assert (ref == np.floor(ref)).mean() == 0.5 and len(voxel_down_sample(f, v)) == 5 ** 3
    # identical points: one voxel, the centroid is the point itself
    f = cc["identical"][0][0]
    np.testing.assert_array_equal(voxel_down_sample(f, C.V), f[:1].astype(np.float64))
    # one voxel of 5,000 points whose sum depends on the order of summation
    f = cc["sum_order"][0][0]
    c = voxel_down_sample(f, C.V)
    assert c.shape == (1, 3) and len(f) == 5000
    assert not np.array_equal(c, voxel_down_sample(f[::-1], C.V))
    assert all(abs(f[:, 0].mean()) > 990 for f in cc["far_translated"][0][:2])
    for axis in range(3):
        f = cc["under_limit_axis%d" % axis][0][0]
        idx = np.floor((f.astype(np.float64) - (f.min(0) - C.V / 2)) / C.V)
        assert C.KEY_FIELD - 4 <= idx.max() <= C.KEY_FIELD - 1 and len(voxel_down_sample(f, C.V)) == 2
        g = C.two_clusters(C.KEY_FIELD + 1, axis)                  # the over-range input of the GPU test
        idx = np.floor((g.astype(np.float64) - (g.min(0) - C.V / 2)) / C.V)
        assert idx.max() >= C.KEY_FIELD and len(voxel_down_sample(g, C.V)) == 2


def test_case_properties_counts():
    cc = C.count_cases()
    # corner cells: the two points of a pair lie in cells that differ by +-1 along every axis, all 8 patterns
    case = cc["corner_cells"]
    pats = set()
    for i, j in case.pairs:
        d = np.floor(case.frags[j] / C.R) - np.floor(case.frags[i] / C.R)
        assert (np.abs(d) == 1).all()
        pats.add(tuple(d[0]))
    assert len(pats) == 8
    assert sorted(len(f) for f in cc["ragged_3DMatch"].frags) == [0, 1, 7, 300, 3000]
    assert len(cc["ragged_3DMatch"].pairs) == 25
    # aliasing: nearly every cell key of fragment 0 is also a cell key of fragment 2, 65536 cells away
    case = cc["cell_aliasing"]
    k0 = {tuple(k) for k in C.cell_keys(case.frags[0], C.R)}
    k2 = {tuple(k) for k in C.cell_keys(case.frags[2], C.R)}
    assert len(k0 & k2) > 0.9 * len(k0)
    assert np.floor(case.frags[2][:, 0] / C.R).min() - np.floor(case.frags[0][:, 0] / C.R).max() > C.KEY_FIELD - 20
    exp = C.expected_counts("cell_aliasing")
    assert exp[0].min() > 100                                       # the true pair does overlap
    # hash load: one cell per point
    case = cc["hash_load"]
    assert len({tuple(k) for k in C.cell_keys(case.frags[0], case.radius)}) == len(case.frags[0]) == 3000
    exp = C.expected_counts("hash_load")
    assert 1500 < exp[0, 1] < 2700                                 # the jitter leaves a real mix of hits and misses
    exp = C.expected_counts("ragged_3DMatch")
    assert 0 < exp[4, 0] < 3000 and exp.max() == 3000              # partial overlaps beside the full self pair
