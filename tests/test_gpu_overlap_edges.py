"""The overlap gate's kernels (csrc/overlap.hip: mvr_voxel_centroids, mvr_radius_index_build,
mvr_radius_overlap_count; the index of csrc/rindex.hpp that mvr_icp_refine shares) at ragged and boundary shapes,
against oracle/overlap.py, which tests/test_overlap_host.py pins on the same inputs (tests/overlap_cases.py) against
brute force.  Centroids bit-equal after a lexsort, counts exact: no tolerance anywhere."""
import warnings

import numpy as np
import pytest

import overlap_cases as C

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- voxel centroids
@pytest.mark.parametrize("name", sorted(C.centroid_cases()))
def test_voxel_centroids_edges(gpu, name):
    from lib.overlap import FragmentOverlap
    from oracle.overlap import voxel_down_sample
    frags, v = C.centroid_cases()[name]
    fo = FragmentOverlap(frags, "FCGF", v)
    ref = [voxel_down_sample(f, v) for f in frags]
    np.testing.assert_array_equal(np.diff(fo.off), [len(o) for o in ref])
    assert fo.off[0] == 0
    c = fo.xyz.cpu().numpy()
    assert c.shape == (fo.off[-1], 3)
    for b, o in enumerate(ref):
        np.testing.assert_array_equal(C.lexsorted(c[fo.off[b]:fo.off[b + 1]]), C.lexsorted(o), err_msg="fragment %d" % b)
    if name == "identical":                 # one voxel, and the centroid equals the point
        np.testing.assert_array_equal(c[:1], frags[0][:1].astype(np.float64))
        assert list(np.diff(fo.off)) == [1, 1]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_voxel_extent_over_range_raises(gpu, axis):
    """Two clusters 65,537 voxels apart: the far cluster's voxel index does not fit the key's 16-bit field.  Before
    the range check, pack_key's mask folded it onto index 1 of the same fragment (read from voxel_key_kernel and
    pack_key; never run on a GPU in that state).  Now a clear error naming the limit, raised from host-side
    validation of a flag the key kernel sets."""
    from lib.overlap import FragmentOverlap, MAX_VOXELS_PER_AXIS
    assert MAX_VOXELS_PER_AXIS == C.KEY_FIELD - 1
    small = np.random.default_rng(axis).uniform(0, 0.2, (50, 3)).astype(np.float32)
    with pytest.raises((ValueError, RuntimeError), match=r"65535 voxels"):
        FragmentOverlap([small, C.two_clusters(C.KEY_FIELD + 1, axis), small], "FCGF", C.V)


# ------------------------------------------------------------------------------------------- index and counts
def _overlap(case):
    from lib.overlap import FragmentOverlap
    return FragmentOverlap(case.frags, case.method, case.voxel, radius=case.radius)


@pytest.mark.parametrize("name", sorted(C.count_cases()))
def test_counts_edges(gpu, name):
    case = C.count_cases()[name]
    exp = C.expected_counts(name)
    fo = _overlap(case)
    assert fo.r == case.r
    got = fo.counts(case.pairs, case.trans)
    assert got.shape == exp.shape
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, "pairs %s: got %s, expected %s" % (case.pairs[bad].tolist(), got[bad].tolist(),
                                                              exp[bad].tolist())
    for k, e in case.expect.items():        # the answers known without the oracle
        assert tuple(got[k]) == tuple(e), (name, k)


@pytest.mark.parametrize("method", ["3DMatch", "FCGF"])
def test_ragged_self_and_empty_pairs(gpu, method):
    """A self pair under the identity reports (n_i, n_i) (for 'FCGF': its voxels); a pair with an empty side (0, 0)."""
    case = C.count_cases()["ragged_" + method]
    fo = _overlap(case)
    n = np.diff(fo.off)
    got = fo.counts(case.pairs, case.trans)
    seen_self = seen_empty = 0
    for k, (i, j) in enumerate(case.pairs):
        if n[i] == 0 or n[j] == 0:
            assert tuple(got[k]) == (0, 0)
            seen_empty += 1
        elif i == j and np.array_equal(case.trans[k], np.eye(4)):
            assert tuple(got[k]) == (n[i], n[i])
            seen_self += 1
    assert seen_self == 3 and seen_empty == 9


@pytest.mark.parametrize("method", ["3DMatch", "FCGF"])
def test_ratios_with_an_empty_side(gpu, method):
    """0.0 beside an empty fragment and no warning (the reference would divide by zero: stated behaviour of
    lib/overlap.py); every other ratio is the reference's max(m01 / n_i, m10 / n_j) on the oracle's counts."""
    case = C.count_cases()["ragged_" + method]
    exp = C.expected_counts("ragged_" + method)
    fo = _overlap(case)
    n = np.diff(fo.off)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ratios = fo.ratios(case.pairs, case.trans)
    assert ratios.dtype == np.float64 and ratios.shape == (len(case.pairs),)
    for k, (i, j) in enumerate(case.pairs):
        if n[i] == 0 or n[j] == 0:
            assert ratios[k] == 0.0
        else:
            assert ratios[k] == max(exp[k, 0] / n[i], exp[k, 1] / n[j])
    assert np.isfinite(ratios).all() and ratios.max() == 1.0


def test_one_pair_and_no_pair(gpu):
    case = C.count_cases()["ragged_3DMatch"]
    exp = C.expected_counts("ragged_3DMatch")
    fo = _overlap(case)
    k = 4                                   # (0, 4): 3000 against 300 points
    got = fo.counts(case.pairs[k:k + 1], case.trans[k:k + 1])
    assert got.shape == (1, 2) and tuple(got[0]) == tuple(exp[k])
    none = fo.counts(np.zeros((0, 2), np.int64), np.zeros((0, 4, 4)))
    assert none.shape == (0, 2)
    assert fo.ratios(np.zeros((0, 2), np.int64), np.zeros((0, 4, 4))).shape == (0,)


def test_all_fragments_empty(gpu):
    """Nothing to index: offsets all 0, counts (0, 0), ratio 0.0, for both methods."""
    from lib.overlap import FragmentOverlap
    for method in ("FCGF", "3DMatch"):
        fo = FragmentOverlap([np.zeros((0, 3), np.float32)] * 3, method, C.V)
        assert list(fo.off) == [0, 0, 0, 0] and fo.M == 0
        assert fo.counts([[0, 1], [2, 2]], [np.eye(4)] * 2).tolist() == [[0, 0], [0, 0]]
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert fo.ratios([[0, 1]], [np.eye(4)]).tolist() == [0.0]
