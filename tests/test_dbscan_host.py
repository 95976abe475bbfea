"""Host side of the DBSCAN clustering (no GPU): the numpy oracle (tests/dbscan_oracle.py) on inputs worked by hand and
against sklearn where it is installed, the conditions every case of tests/test_gpu_dbscan.py relies on (asserted here
on the oracle, so a GPU test cannot pass by luck), the argument checks that need no device, the --denoise parser, and
the C entry point's argument rules where it returns before any HIP call."""
import inspect
import os

import numpy as np
import pytest

import dbscan_oracle as D
import knn_oracle as K
from conftest import PKG

LIB = os.path.join(PKG, "libmvreg_hip.so")


def _run(points, eps, min_points, off=None):
    xyz = np.asarray(points, np.float64).reshape(-1, 3)
    return D.dbscan(xyz, np.array([0, len(xyz)] if off is None else off), eps, min_points)


def _line(xs):
    return [[x, 0.0, 0.0] for x in xs]


# ------------------------------------------------------------------------------------------ the oracle, by hand
def test_oracle_chain_with_a_pair_at_exactly_eps():
    # 0 - 1 - 2 are 1 apart, 4 is exactly 2 from 2: with eps = 2 (strict) it is nobody's neighbour
    res = _run(_line([0.0, 1.0, 2.0, 4.0]), 2.0, 2)
    assert res["core"].tolist() == [True, True, True, False]
    assert res["labels"].tolist() == [0, 0, 0, -1] and res["n_clusters"].tolist() == [1]
    assert res["sizes"].tolist() == [3, 0, 0, 0]
    assert res["labels"].dtype == np.int32 and res["sizes"].dtype == np.int32 and res["core"].dtype == bool
    assert res["n_clusters"].dtype == np.int64
    # just above eps the pair joins
    assert _run(_line([0.0, 1.0, 2.0, 4.0]), 2.0000001, 2)["labels"].tolist() == [0, 0, 0, 0]
    assert D.margin(np.asarray(_line([0.0, 1.0, 2.0, 4.0])), np.array([0, 4]), 2.0) == 0.0


# a core with three satellites 0.9 from it and more than 1 from each other: at eps = 1, min_points = 4 only the centre
# is core.  _A around the origin, _B around (1.8, 0, 0); _MID is 0.9 from both centres and from nothing else
_A = [[0.0, 0, 0], [-0.9, 0, 0], [0.0, 0.9, 0], [0.0, -0.9, 0]]
_B = [[1.8, 0, 0], [2.7, 0, 0], [1.8, 0.9, 0], [1.8, -0.9, 0]]
_MID = [[0.9, 0, 0]]


def test_oracle_border_between_two_clusters_takes_the_lower_number():
    res = _run(_A + _B + _MID, 1.0, 4)
    assert res["core"].tolist() == [True, False, False, False, True, False, False, False, False]
    assert res["labels"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0] and res["n_clusters"].tolist() == [2]
    assert res["sizes"][:3].tolist() == [5, 4, 0]
    # the same points with the other core stored first: the border belongs to what is cluster 0 there
    assert _run(_B + _A + _MID, 1.0, 4)["labels"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0]
    # and wherever the border point is stored itself (the loop marks it noise first, then relabels it)
    assert _run(_MID + _B + _A, 1.0, 4)["labels"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert _run(_A + _MID + _B, 1.0, 4)["labels"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]


def test_oracle_numbering_goes_by_core_rows_not_border_rows():
    # row 0 is a border point of the cluster whose core is row 5; the cluster of core row 1 is number 0 all the same
    res = _run(_A[1:2] + _B + _A[:1] + _A[2:], 1.0, 4)
    assert res["core"].tolist() == [False, True, False, False, False, True, False, False]
    assert res["labels"].tolist() == [1, 0, 0, 0, 0, 1, 1, 1] and res["n_clusters"].tolist() == [2]
    assert res["sizes"].tolist() == [4, 4, 0, 0, 0, 0, 0, 0]


def test_oracle_min_points_one_and_duplicates():
    res = _run(_line([0.0, 5.0, 5.5, 9.0]), 1.0, 1)          # every point is core, singletons are clusters
    assert res["core"].all() and res["labels"].tolist() == [0, 1, 1, 2] and res["sizes"].tolist() == [1, 2, 1, 0]
    # a point stored three times is a core of min_points = 3 by itself
    pts = [[1.0, 1, 1], [0.0, 0, 0], [1.0, 1, 1], [1.0, 1, 1]]
    res = _run(pts, 0.1, 3)
    assert res["core"].tolist() == [True, False, True, True] and res["labels"].tolist() == [0, -1, 0, 0]
    assert _run(pts, 0.1, 4)["labels"].tolist() == [-1] * 4


def test_oracle_offsets_with_an_empty_and_a_one_point_fragment():
    pts = [[5.0, 5, 5]] + _line([0.0, 0.1, 0.2]) + _line([0.0, 0.1])
    res = _run(pts, 0.15, 2, off=[0, 0, 1, 4, 6])
    assert res["n_clusters"].tolist() == [0, 0, 1, 1]
    assert res["labels"].tolist() == [-1, 0, 0, 0, 0, 0]           # numbers restart in every fragment
    assert res["sizes"].tolist() == [0, 3, 0, 0, 2, 0] and res["core"].tolist() == [False] + [True] * 5
    keep = D.cluster_keep(res, [0, 0, 1, 4, 6], min_size=3)
    assert keep.tolist() == [False, True, True, True, False, False]
    assert D.cluster_keep(res, [0, 0, 1, 4, 6], largest=True).tolist() == [False] + [True] * 5


def test_oracle_largest_cluster_tie_keeps_the_lower_number():
    res = _run(_line([0.0, 0.1, 5.0, 5.1, 9.0]), 0.2, 2)
    assert res["labels"].tolist() == [0, 0, 1, 1, -1]
    assert D.cluster_keep(res, [0, 5], largest=True).tolist() == [True, True, False, False, False]


# ------------------------------------------------------------------------------------------------ sklearn
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_oracle_equals_sklearn(name):
    cluster = pytest.importorskip("sklearn.cluster")
    frags, _, eps, min_points = D.CASES[name]()
    xyz, off, res = D.case_oracle(name)
    for b in range(len(off) - 1):
        X = xyz[off[b]:off[b + 1]]
        if len(X) == 0:
            continue
        want = cluster.DBSCAN(eps=eps, min_samples=min_points, algorithm="brute").fit(X)
        np.testing.assert_array_equal(res["labels"][off[b]:off[b + 1]], want.labels_)
        core = np.zeros(len(X), bool)
        core[want.core_sample_indices_] = True
        np.testing.assert_array_equal(res["core"][off[b]:off[b + 1]], core)


# ------------------------------------------------------------------------------------- conditions of the GPU cases
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_no_decision_of_a_case_is_within_rounding_of_eps(name):
    frags, r, eps, min_points = D.CASES[name]()
    xyz, off, res = D.case_oracle(name)
    m = D.margin(xyz, off, eps)
    print("%s: %d points, clusters %s, %d noise, margin %.3g" % (name, len(xyz), res["n_clusters"].tolist(),
                                                                (res["labels"] < 0).sum(), m))
    assert m > 1e-9 and eps <= r
    # the outputs agree with each other
    for b in range(len(off) - 1):
        lab, size = res["labels"][off[b]:off[b + 1]], res["sizes"][off[b]:off[b + 1]]
        n = res["n_clusters"][b]
        assert lab.max(initial=-1) == n - 1 and (size[:n] > 0).all() and not size[n:].any()
        assert size.sum() == (lab >= 0).sum() and (lab[res["core"][off[b]:off[b + 1]]] >= 0).all()


def test_conditions_of_the_clouds_case():
    A, B, pa, pb = K.clouds()
    xyz, off, res = D.case_oracle("clouds")
    planted = np.concatenate([pa, pb])
    assert res["n_clusters"].tolist() == [1, 1] and res["sizes"][off[0]] == 2000 and res["sizes"][off[1]] == 1200
    assert (res["labels"][planted] == -1).all() and (res["labels"][~planted] == 0).all()
    assert (xyz < 0).any(0).all()


def test_conditions_of_the_blobs_case():
    xyz, off, res = D.case_oracle("blobs")
    eps = D.blobs_case()[2]
    borders, several = D.multi_cluster_borders(xyz, off, eps, res)
    print("blobs: %d clusters, %d noise, %d border points, %d of them between clusters"
          % (res["n_clusters"][0], (res["labels"] < 0).sum(), borders, several))
    assert len(xyz) == 2400 and several >= 5 and res["n_clusters"][0] >= 2 and (res["labels"] < 0).sum() >= 1
    assert (res["n_clusters"][0], (res["labels"] < 0).sum(), borders, several) == (37, 99, 343, 18)


def test_conditions_of_the_helices_case():
    xyz, off, res = D.case_oracle("helices")
    assert len(xyz) == 6000 and res["n_clusters"].tolist() == [2] and res["sizes"][:3].tolist() == [3000, 3000, 0]
    assert (res["labels"] >= 0).all() and (xyz < 0).any(0).all()
    assert D.margin(xyz, off, 0.05) > 0.1
    # many cells and many workgroups of 64: the chains cross them
    cells = np.unique(np.floor(xyz / 0.075).astype(np.int64), axis=0)
    assert len(cells) > 300


def test_conditions_of_the_ties_and_ragged_cases():
    xyz, off, res = D.case_oracle("ties")
    r = D.ties_case()[1]
    assert (np.floor(xyz / r) * r == xyz).any() and res["n_clusters"].tolist() == [2]
    assert res["sizes"][:2].tolist() == [1763, 8] and (res["labels"] < 0).sum() == 107
    xyz, off, res = D.case_oracle("ragged")
    assert np.diff(off).tolist() == [0, 1, 5, 19, 20, 21] and D.RAGGED_EPS <= K.R_CELL
    assert (res["n_clusters"] > 0).any() and (res["n_clusters"][2:] == 0).any() and res["n_clusters"][:2].tolist() == [0, 0]


@pytest.fixture(scope="module")
def scene_centroids():
    from oracle.overlap import voxel_down_sample
    frags, blobs = D.scene_blob_case()
    flying = K.scene_case()[1]
    out = []
    for f, blob, fly in zip(frags, blobs, flying):
        cen = voxel_down_sample(f, 0.025)
        near = lambda p: np.sqrt(((cen[:, None, :] - p.astype(np.float64)[None]) ** 2).sum(2)).min(1)   # noqa: E731
        out.append((cen, near(blob) < 0.0434, near(fly) < 1e-6))       # 0.0434: above a voxel's diagonal
    return out


def test_conditions_of_the_scene_case(scene_centroids):
    spec = D.SCENE_SPEC
    for b, (cen, is_blob, is_flying) in enumerate(scene_centroids):
        off = np.array([0, len(cen)])
        surface = ~is_blob & ~is_flying
        count, m_radius = K.radius_count(cen, off, 0.075, with_margin=True)
        kept_by_radius = (count[is_blob] > 16).mean()                 # radius_outliers at its defaults
        res = D.dbscan(cen, off, 0.075, spec["min_points"])
        keep = D.cluster_keep(res, off, min_size=spec["min_size"])
        print("fragment %d: %d centroids, %d of the blob; the radius filter keeps %.0f %% of it, the cluster filter %d "
              "of it and removes %d of %d surface centroids; clusters of %s"
              % (b, len(cen), is_blob.sum(), 100 * kept_by_radius, keep[is_blob].sum(), (~keep[surface]).sum(),
                 surface.sum(), res["sizes"][:res["n_clusters"][0]].tolist()))
        assert is_blob.sum() >= 10 and is_flying.sum() == K.N_SCENE_PLANTED and m_radius > 1e-9
        assert kept_by_radius > 0.5
        assert not keep[is_blob].any() and (~keep[surface]).sum() <= 0.01 * surface.sum()


# ------------------------------------------------------------------------------------------------ argument helpers
def test_dbscan_arguments():
    from lib import overlap as V
    assert V._dbscan_arguments(None, 10, 0.075) == (0.075, 10)
    assert V._dbscan_arguments(0.05, 1, 0.075) == (0.05, 1)
    assert V._dbscan_arguments(0.075, np.int64(3), 0.075) == (0.075, 3)
    for eps in (0.0, -0.1, 0.0751, float("nan"), float("inf"), "0.05", True):
        with pytest.raises(ValueError, match="cluster_dbscan: eps"):
            V._dbscan_arguments(eps, 10, 0.075)
    for mp in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="cluster_dbscan: min_points"):
            V._dbscan_arguments(0.05, mp, 0.075)
    assert V._cluster_keep_arguments(100, False) == (100, False)
    assert V._cluster_keep_arguments(None, True) == (None, True)
    for min_size, largest in ((None, False), (10, True), (0, False), (-1, False), (2.5, False), (True, False),
                              (10, 1)):
        with pytest.raises(ValueError, match="cluster_keep"):
            V._cluster_keep_arguments(min_size, largest)
    sig = inspect.signature(V.FragmentOverlap.cluster_dbscan).parameters
    assert sig["eps"].default is None and sig["min_points"].default == 10
    sig = inspect.signature(V.FragmentOverlap.cluster_keep).parameters
    assert sig["min_size"].default is None and sig["largest"].default is False


def test_cluster_method_of_the_denoise_argument():
    from lib import multiview as MV
    assert MV.DENOISE_METHODS["cluster"] == {"min_points": 10, "min_size": 100, "eps": None}
    assert set(MV.DENOISE_METHODS) == {"statistical", "radius", "cluster"}
    assert MV._denoise_arguments({"method": "cluster"}) == {"method": "cluster", "min_points": 10, "min_size": 100,
                                                            "eps": None}
    assert MV._denoise_arguments({"method": "cluster"}, 0.075) == {"method": "cluster", "min_points": 10,
                                                                   "min_size": 100, "eps": None}
    assert MV._denoise_arguments({"method": "cluster", "min_points": 5, "min_size": 30, "eps": 0.05}, 0.075) == {
        "method": "cluster", "min_points": 5, "min_size": 30, "eps": 0.05}
    for bad in ({"method": "cluster", "eps": 0.0751}, {"method": "cluster", "eps": 0.0},
                {"method": "cluster", "eps": float("nan")}, {"method": "cluster", "min_points": 0},
                {"method": "cluster", "min_size": 0}, {"method": "cluster", "min_size": 2.5},
                {"method": "cluster", "radius": 0.05}, {"method": "cluster", "nb_points": 3},
                {"method": "radius", "eps": 0.05}):
        with pytest.raises(ValueError):
            MV._denoise_arguments(bad, 0.075)
    # the two earlier methods are as they were
    assert MV._denoise_arguments({"method": "radius"}, 0.075) == {"method": "radius", "nb_points": 16, "radius": None}
    assert MV._denoise_arguments({"method": "statistical"}) == {"method": "statistical", "nb_neighbors": 20,
                                                                "std_ratio": 2.0}
    # the checks come before any device work: no fragment is looked at
    with pytest.raises(ValueError, match="min_points"):
        MV.register_scene([None, None], 0.025, denoise={"method": "cluster", "min_points": 0})
    with pytest.raises(ValueError, match="eps"):
        MV.register_scene([None, None], 0.025, denoise={"method": "cluster", "eps": 0.076})


def test_cluster_form_of_the_cli_option():
    from scripts import register_scene as S
    assert S.parse_denoise("cluster:10:100") == {"method": "cluster", "min_points": 10, "min_size": 100, "eps": None}
    assert S.parse_denoise("cluster:10:100:0.05") == {"method": "cluster", "min_points": 10, "min_size": 100,
                                                      "eps": 0.05}
    assert S.parse_denoise("radius:16") == {"method": "radius", "nb_points": 16, "radius": None}
    for bad in ("cluster", "cluster:10", "cluster:10:100:0.05:1", "cluster:x:100", "cluster:10:1.5", "cluster:10:100:e",
                "clusters:10:100"):
        with pytest.raises(ValueError, match="--denoise must be"):
            S.parse_denoise(bad)
    ap = S.parser()
    base = ["--fragments", "a.ply", "b.ply", "--out", "o"]
    a = S.check_args(ap, ap.parse_args(base + ["--denoise", "cluster:10:100"]))
    assert a.denoise == {"method": "cluster", "min_points": 10, "min_size": 100, "eps": None}
    a = S.check_args(ap, ap.parse_args(base + ["--denoise", "cluster:5:30:0.06"]))
    assert a.denoise == {"method": "cluster", "min_points": 5, "min_size": 30, "eps": 0.06}
    for spec in ("cluster:0:100", "cluster:10:0", "cluster:10:100:0.08", "cluster:10:100:0"):    # 0.08 > 3 voxels
        with pytest.raises(SystemExit):
            S.check_args(ap, ap.parse_args(base + ["--denoise", spec]))


# ------------------------------------------------------------------------------------------- the ABI without a GPU
_Z = None


def _call(L, M=0, r=0.05, eps=0.05, min_points=10, B=2):
    return L.mvr_cluster_dbscan(_Z, 0, _Z, _Z, B, M, r, eps, min_points, _Z, _Z, _Z, _Z, _Z, 0, _Z)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")
def test_entry_point_without_a_device():
    from lib import _native
    L = _native.lib()
    assert "mvr_cluster_dbscan" in _native.EXPORTS and "mvr_dbscan_workspace_bytes" in _native.EXPORTS
    assert _call(L) == 0                                                    # M == 0: MVR_OK with NULL pointers
    assert _call(L, eps=0.01) == 0 and _call(L, min_points=1) == 0
    # scalars are checked before the empty short-cut
    assert _call(L, eps=0.0500001) == -1 and _call(L, min_points=0) == -1 and _call(L, eps=float("nan")) == -1
    assert _call(L, eps=0.0) == -1 and _call(L, r=0.0) == -1 and _call(L, M=-1) == -1 and _call(L, M=1 << 31) == -1
    assert _call(L, B=0) == -1 and _call(L, B=1 << 15) == -1 and _call(L, min_points=-3) == -1
    assert _call(L, M=10) == -1                                             # with points every pointer is needed
    sizes = [L.mvr_dbscan_workspace_bytes(M) for M in (0, 1, 63, 64, 1000, 4096, 4097, 100000, 612000)]
    assert sizes[0] >= 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[4] >= 4 * 4 * 1001 and sizes[-1] >= 4 * 4 * 612001
