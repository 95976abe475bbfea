"""Host side of the k-nearest-neighbour search and the outlier filters (no GPU): the numpy oracle
(tests/knn_oracle.py) on inputs computed by hand, the conditions every case of tests/test_gpu_knn.py relies on
(asserted here on the oracle, so a GPU test cannot pass by luck), the argument checks that need no device, the
--denoise parser, and the C entry points' argument rules where they return before any HIP call."""
import inspect
import os

import numpy as np
import pytest

import knn_oracle as K
from conftest import PKG

LIB = os.path.join(PKG, "libmvreg_hip.so")
INF = float("inf")


# ------------------------------------------------------------------------------------------ the oracle, by hand
def test_oracle_collinear_points():
    xyz = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    off = np.array([0, 4])
    idx, d2 = K.knn_self(xyz, off, 3)
    assert idx.tolist() == [[0, 1, 2], [1, 0, 2], [2, 1, 0], [3, 2, 1]]
    assert d2.tolist() == [[0, 1, 9], [0, 1, 4], [0, 4, 9], [0, 16, 36]]
    assert idx.dtype == np.int32 and d2.dtype == np.float64
    st = K.statistical(d2, off, 3, 1.0)
    means = np.array([4.0, 3.0, 5.0, 10.0]) / 3.0
    np.testing.assert_allclose(st["mean_dist"], means, rtol=1e-15)
    mu, sd = 22.0 / 12.0, np.sqrt(((means - 22.0 / 12.0) ** 2).sum() / 3.0)
    np.testing.assert_allclose(st["threshold"], [mu + sd], rtol=1e-15)
    assert st["keep"].tolist() == [True, True, True, False]
    assert K.radius_count(xyz, off, 2.5).tolist() == [2, 3, 2, 1]
    assert K.radius_count(xyz, off, 2.0).tolist() == [2, 2, 1, 1]          # strict: the pair at exactly 2 is out


def test_oracle_fragment_smaller_than_k_and_offsets():
    xyz = np.array([[5.0, 5, 5], [0.0, 0, 0], [0.0, 0, 2], [0.0, 1, 0]])
    off = np.array([0, 0, 1, 4])                                            # an empty fragment, one point, three
    idx, d2 = K.knn_self(xyz, off, 4)
    assert idx.tolist() == [[0, -1, -1, -1], [1, 3, 2, -1], [2, 1, 3, -1], [3, 1, 2, -1]]   # global rows
    assert d2.tolist() == [[0, INF, INF, INF], [0, 1, 4, INF], [0, 4, 5, INF], [0, 1, 5, INF]]
    st = K.statistical(d2, off, 4, 2.0)
    np.testing.assert_allclose(st["mean_dist"], [0, 1.0, (2 + np.sqrt(5)) / 3, (1 + np.sqrt(5)) / 3], rtol=1e-15)
    assert st["threshold"][0] == INF and st["threshold"][1] == INF and st["keep"][0]     # below two points: kept
    assert K.radius_count(xyz, off, 1.5).tolist() == [1, 2, 1, 2]


def test_oracle_duplicates_come_lower_row_first():
    xyz = np.array([[1.0, 1, 1], [0.0, 0, 0], [1.0, 1, 1], [1.0, 1, 1]])
    idx, d2 = K.knn_self(xyz, np.array([0, 4]), 3)
    assert idx.tolist() == [[0, 2, 3], [1, 0, 2], [0, 2, 3], [0, 2, 3]]     # rows 2 and 3 are not their own first
    assert d2.tolist() == [[0, 0, 0], [0, 3, 3], [0, 0, 0], [0, 0, 0]]


# ------------------------------------------------------------------------------------- conditions of the GPU cases
def test_conditions_of_the_statistical_case():
    A, B, pa, pb = K.clouds()
    off, planted = K.offsets([A, B]), np.concatenate([pa, pb])
    assert off.tolist() == [0, 2030, 3260] and planted.sum() == 60 and (K.stack([A, B]) < 0).any(0).all()
    _, d2 = K.clouds_knn(K.K_STAT)
    st = K.statistical(d2, off, K.K_STAT, K.STD_RATIO)
    thr = np.repeat(st["threshold"], np.diff(off))
    margin = np.abs(st["mean_dist"] - thr) / thr
    print("statistical case: %d of 60 planted removed, %d surface points removed, closest margin %.3g"
          % ((~st["keep"] & planted).sum(), (~st["keep"] & ~planted).sum(), margin.min()))
    assert margin.min() > 1e-6
    assert not st["keep"][planted].any()
    assert (~st["keep"] & ~planted).sum() <= 0.01 * (~planted).sum()


def test_conditions_of_the_radius_case():
    A, B, pa, pb = K.clouds()
    off, planted = K.offsets([A, B]), np.concatenate([pa, pb])
    count, margin = K.radius_count(K.stack([A, B]), off, K.R_CELL, with_margin=True)
    print("radius case: planted count <= %d, surface count >= %d, |d - radius| / radius >= %.3g"
          % (count[planted].max(), count[~planted].min(), margin))
    assert count[planted].max() <= 2 and count[~planted].min() >= 15
    assert not np.isin(count, [K.NB_POINTS, K.NB_POINTS + 1]).any()
    assert margin > 1e-9            # no decision within rounding of the radius, whatever the rounding of d


def test_conditions_of_the_knn_cases():
    A, B = K.clouds()[:2]
    xyz, off = K.stack([A, B]), K.offsets([A, B])
    ring = K.resolving_ring(xyz, off, K.K_STAT, K.R_CELL)
    n1, n2, n0 = (ring == 1).sum(), (ring == 2).sum(), (ring == 0).sum()
    print("k = 20 on the two clouds: %d queries settled by ring 1, %d by ring 2, %d by the direct scan" % (n1, n2, n0))
    assert n1 > 0.9 * len(xyz) and n2 > 0 and n0 > 0
    ring64 = K.resolving_ring(xyz, off, 64, K.R_CELL)
    assert (ring64 == 2).sum() > 100                                        # k = 64 mostly needs the second ring
    frags, r, k = K.sparse_case()
    assert (K.resolving_ring(K.stack(frags), K.offsets(frags), k, r) == 0).mean() > 0.9
    iso = K.isolated_case()[0]
    far = np.linalg.norm(iso[-5:] - A.mean(0), axis=1)
    assert len(iso) == len(A) + 5 and (far >= 4.0).all() and (far <= 6.0).all()
    assert (K.resolving_ring(iso, K.offsets([iso]), K.K_STAT, K.R_CELL)[-5:] == 0).all()
    assert [len(f) for f in K.ragged_case()] == [0, 1, 5, 19, 20, 21]
    # ties: coordinates on cell faces, exactly equal distances, exact duplicates
    frags, r = K.ties_case()
    pts = frags[0]
    assert len(pts) == 12 ** 3 + 150 and (np.floor(pts / r) * r == pts).any()
    idx, d2 = K.knn_self(pts, K.offsets(frags), K.K_STAT)
    assert (d2[:, 1:] == d2[:, :-1]).mean() > 0.5                           # most neighbours tie with the one before
    assert (d2[:, 2] == 0).sum() == 150 and (idx[:, 0] != np.arange(len(pts))).sum() == 100


def test_conditions_of_the_scene_case():
    import icp_oracle as O
    from oracle.overlap import voxel_down_sample
    frags, flying = K.scene_case()
    for b, (f, p) in enumerate(zip(frags, flying)):
        assert len(f) == len(O.scene4()[0][b]) + K.N_SCENE_PLANTED
        cen = voxel_down_sample(f, 0.025)
        off = np.array([0, len(cen)])
        st = K.statistical(K.knn_self(cen, off, K.K_STAT)[1], off, K.K_STAT, K.STD_RATIO)
        d = np.sqrt(((cen[:, None, :] - p.astype(np.float64)[None]) ** 2).sum(2))
        own = d.argmin(0)                                                   # each flying pixel is a centroid of its own
        margin = np.abs(st["mean_dist"] - st["threshold"][0]).min() / st["threshold"][0]
        print("fragment %d: %d centroids, %d removed, closest margin %.3g" % (b, len(cen), (~st["keep"]).sum(), margin))
        assert d.min(0).max() < 1e-6 and not st["keep"][own].any() and margin > 1e-6
        assert (~st["keep"]).sum() <= K.N_SCENE_PLANTED + 0.01 * len(cen)


# ------------------------------------------------------------------------------------------------ argument helpers
def test_knn_and_filter_arguments():
    from lib import overlap as V
    assert V._knn_arguments(1) == 1 and V._knn_arguments(64) == 64 and V.MAX_KNN == 64
    for k in (0, 65, -3, 2.5, True):
        with pytest.raises(ValueError, match="knn: k"):
            V._knn_arguments(k)
    assert V._statistical_arguments(20, 2) == (20, 2.0)
    for nb, ratio in ((0, 2.0), (65, 2.0), (20, 0.0), (20, -1.0), (20, float("nan")), (1.5, 2.0)):
        with pytest.raises(ValueError, match="statistical_outliers"):
            V._statistical_arguments(nb, ratio)
    assert V._radius_outlier_arguments(16, None, 0.075) == (16, 0.075)
    assert V._radius_outlier_arguments(0, 0.05, 0.075) == (0, 0.05)
    for radius in (0.0, -0.1, 0.0751, float("nan")):
        with pytest.raises(ValueError, match=r"radius_outliers: radius .* must lie in \(0, 0.075\], the index's cell"):
            V._radius_outlier_arguments(16, radius, 0.075)
    with pytest.raises(ValueError, match="nb_points"):
        V._radius_outlier_arguments(-1, None, 0.075)
    import torch
    m = V._keep_mask(np.array([1, 0, 1], np.uint8), 3)
    assert m.dtype == torch.bool and m.tolist() == [True, False, True]
    assert V._keep_mask(torch.tensor([True, False]), 2).tolist() == [True, False]
    for bad, M in ((np.zeros(3, bool), 4), (np.zeros(3, np.int64), 3), (np.zeros((3, 1), bool), 3),
                   (np.zeros(3, np.float32), 3)):
        with pytest.raises(ValueError, match="select: keep"):
            V._keep_mask(bad, M)
    for name in ("knn", "statistical_outliers", "radius_outliers", "select"):
        assert callable(getattr(V.FragmentOverlap, name))
    sig = inspect.signature(V.FragmentOverlap.statistical_outliers).parameters
    assert sig["nb_neighbors"].default == 20 and sig["std_ratio"].default == 2.0
    sig = inspect.signature(V.FragmentOverlap.radius_outliers).parameters
    assert sig["nb_points"].default == 16 and sig["radius"].default is None


def test_denoise_argument_of_register_scene():
    from lib import multiview as MV
    assert inspect.signature(MV.register_scene).parameters["denoise"].default is None
    assert MV._denoise_arguments(None) is None
    assert MV._denoise_arguments({"method": "statistical"}) == {"method": "statistical", "nb_neighbors": 20,
                                                                "std_ratio": 2.0}
    assert MV._denoise_arguments({"method": "statistical", "nb_neighbors": 8, "std_ratio": 1}, 0.075) == {
        "method": "statistical", "nb_neighbors": 8, "std_ratio": 1.0}
    assert MV._denoise_arguments({"method": "radius"}, 0.075) == {"method": "radius", "nb_points": 16, "radius": None}
    assert MV._denoise_arguments({"method": "radius", "nb_points": 4, "radius": 0.05}, 0.075) == {
        "method": "radius", "nb_points": 4, "radius": 0.05}
    for bad in ("statistical", {}, {"nb_neighbors": 20}, {"method": "median"}, {"method": "statistical", "radius": 1},
                {"method": "radius", "std_ratio": 2.0}, {"method": "statistical", "nb_neighbors": 0},
                {"method": "statistical", "nb_neighbors": 65}, {"method": "statistical", "std_ratio": 0.0},
                {"method": "radius", "radius": 0.08}, {"method": "radius", "radius": 0.0},
                {"method": "radius", "nb_points": -1}):
        with pytest.raises(ValueError):
            MV._denoise_arguments(bad, 0.075)
    # the checks come before any device work: no fragment is looked at
    with pytest.raises(ValueError, match="denoise"):
        MV.register_scene([None, None], 0.025, denoise={"method": "median"})


def test_denoise_option_of_the_cli():
    from scripts import register_scene as S
    assert S.parse_denoise("statistical:20:2.0") == {"method": "statistical", "nb_neighbors": 20, "std_ratio": 2.0}
    assert S.parse_denoise("radius:16") == {"method": "radius", "nb_points": 16, "radius": None}
    assert S.parse_denoise("radius:8:0.05") == {"method": "radius", "nb_points": 8, "radius": 0.05}
    for bad in ("", "statistical", "statistical:20", "statistical:20:2.0:1", "statistical:x:2.0", "statistical:20:y",
                "radius", "radius:1.5", "radius:16:0.05:3", "median:3:1"):
        with pytest.raises(ValueError, match="--denoise must be"):
            S.parse_denoise(bad)
    ap = S.parser()
    base = ["--fragments", "a.ply", "b.ply", "--out", "o"]
    assert S.check_args(ap, ap.parse_args(base)).denoise is None
    a = S.check_args(ap, ap.parse_args(base + ["--denoise", "statistical:20:2.0"]))
    assert a.denoise == {"method": "statistical", "nb_neighbors": 20, "std_ratio": 2.0}
    a = S.check_args(ap, ap.parse_args(base + ["--denoise", "radius:16:0.06"]))
    assert a.denoise == {"method": "radius", "nb_points": 16, "radius": 0.06}
    for spec in ("statistical:0:2.0", "statistical:65:2.0", "statistical:20:0", "radius:16:0.08", "radius:-1",
                 "nonsense"):                                               # 0.08 > 3 voxels of 0.025
        with pytest.raises(SystemExit):
            S.check_args(ap, ap.parse_args(base + ["--denoise", spec]))


# ------------------------------------------------------------------------------------------- the ABI without a GPU
_Z = None
_KNN = lambda L, M=0, r=0.05, k=20: L.mvr_knn_self(_Z, 0, _Z, _Z, 2, M, r, k, _Z, _Z, _Z, 0, _Z)          # noqa: E731
_STAT = lambda L, M=0, k=20, ratio=2.0: L.mvr_statistical_outlier(_Z, _Z, 2, M, k, ratio, _Z, _Z, _Z, _Z)  # noqa: E731
_COUNT = lambda L, M=0, r=0.05, radius=0.05: L.mvr_radius_count(_Z, 0, _Z, _Z, 2, M, r, radius, _Z, _Z)    # noqa: E731


@pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")
def test_entry_points_without_a_device():
    from lib import _native
    L = _native.lib()
    for name in ("mvr_knn_self_workspace_bytes", "mvr_knn_self", "mvr_statistical_outlier", "mvr_radius_count"):
        assert name in _native.EXPORTS
    assert L.mvr_knn_self_workspace_bytes(1000) >= 4 * 1000 + 4 and L.mvr_knn_self_workspace_bytes(0) > 0
    # M == 0: MVR_OK with NULL pointers
    assert _KNN(L) == 0 and _STAT(L) == 0 and _COUNT(L) == 0
    # scalars are checked before the empty short-cut
    assert _KNN(L, k=0) == -1 and _KNN(L, k=65) == -1 and _KNN(L, r=0.0) == -1 and _KNN(L, r=-1.0) == -1
    assert _KNN(L, r=float("nan")) == -1 and _KNN(L, M=-1) == -1 and _KNN(L, M=1 << 31) == -1
    assert _KNN(L, k=1) == 0 and _KNN(L, k=64) == 0
    assert _STAT(L, k=0) == -1 and _STAT(L, k=65) == -1 and _STAT(L, ratio=0.0) == -1 and _STAT(L, ratio=-2.0) == -1
    assert _STAT(L, ratio=float("nan")) == -1 and _STAT(L, M=-1) == -1
    assert _COUNT(L, r=0.0) == -1 and _COUNT(L, radius=0.0) == -1 and _COUNT(L, r=0.05, radius=0.0500001) == -1
    assert _COUNT(L, M=-1) == -1 and _COUNT(L, radius=0.01) == 0
    assert L.mvr_knn_self(_Z, 0, _Z, _Z, 0, 0, 0.05, 20, _Z, _Z, _Z, 0, _Z) == -1          # B == 0
    assert L.mvr_knn_self(_Z, 0, _Z, _Z, 1 << 15, 0, 0.05, 20, _Z, _Z, _Z, 0, _Z) == -1
    # with points every pointer is needed
    assert _KNN(L, M=10) == -1 and _STAT(L, M=10) == -1 and _COUNT(L, M=10) == -1
