"""CPU-side checks of the FPFH descriptors and the feature matcher: the properties of the oracle
(tests/fpfh_oracle.py), the input conditions the GPU comparisons of test_gpu_fpfh.py rest on (the share of rows whose
histogram is decided by rounding stays within its cap on the scene, and is zero on the random shapes), the Python
surface's argument errors and the three entry points' validation (returns before any HIP call)."""
import os
import types

import numpy as np
import pytest

from conftest import PKG
import icp_oracle as O
import icp_plane_oracle as PO
import fpfh_oracle as FO

LIB = os.path.join(PKG, "libmvreg_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")


# ---------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("radius", FO.SCENE_RADII)
def test_scene_rows_sum_and_stay_within_the_caps(radius):
    """The caps come from a CPU prototype on these very inputs (0.22 % / 0.40 % of the SPFH rows and 4.3 % / 2.6 %
    of the FPFH rows of fragments 0 / 1 unsafe at radius 0.075, all of them exact symmetric ties of the centroid
    lattice at the room's edges): SPFH <= 0.01, FPFH <= 0.06."""
    frags, _, _, res = FO.scene_case(radius)
    for b, r in zip(FO.SCENE_FRAGS, res):
        has = r["k"] > 0
        print("fragment %d, radius %g: %d points, k %d..%d, unsafe SPFH %.4f, FPFH %.4f"
              % (b, radius, len(r["k"]), r["k"].min(), r["k"].max(), r["unsafe_spfh"].mean(),
                 r["unsafe_fpfh"].mean()))
        assert has.mean() > 0.99 and r["k"].max() < 2 ** 16
        groups = r["spfh"][has].reshape(-1, 3, 11).sum(2)
        np.testing.assert_allclose(groups, 100.0, rtol=0, atol=1e-9)        # every pair of the scene is binned
        np.testing.assert_allclose(r["fpfh"][has].sum(1), 600.0, rtol=0, atol=1e-9)
        assert (r["spfh"] >= 0).all() and (r["fpfh"] >= 0).all()
        assert r["unsafe_spfh"].mean() <= FO.CAP_SPFH and r["unsafe_fpfh"].mean() <= FO.CAP_FPFH


def test_rigid_motion_leaves_the_safe_rows_unchanged():
    """points, normals and viewpoint moved together: the normals are re-estimated on the moved points"""
    frags, normals, vps, res = FO.scene_case(0.075)
    T = O.rigid([0.3, -1.0, 0.5], 37.0, [0.4, -0.7, 0.2])
    R, t = T[:3, :3], T[:3, 3]
    for f, n, v, r in zip(frags, normals, vps, res):
        moved = f @ R.T + t
        n2 = PO.estimate_normals(moved, PO.NORMAL_RADIUS, R @ v + t)["normals"]
        assert np.abs(n2 - n @ R.T).max() < 1e-6                             # the same normals, the same signs
        r2 = FO.fpfh(moved, n2, 0.075)
        np.testing.assert_array_equal(r2["k"], r["k"])
        safe_s = ~(r["unsafe_spfh"] | r2["unsafe_spfh"])
        safe_f = ~(r["unsafe_fpfh"] | r2["unsafe_fpfh"])
        ds, df = np.abs(r2["spfh"] - r["spfh"]).max(1), np.abs(r2["fpfh"] - r["fpfh"]).max(1)
        print("moved copy: safe rows SPFH %.4f FPFH %.4f, largest difference on them %.3g / %.3g; rows that differ "
              "at all: %d / %d" % (safe_s.mean(), safe_f.mean(), ds[safe_s].max(), df[safe_f].max(),
                                   int((ds > 1e-9).sum()), int((df > 1e-9).sum())))
        assert safe_s.mean() >= 1 - 2 * FO.CAP_SPFH and safe_f.mean() >= 1 - 2 * FO.CAP_FPFH
        assert ds[safe_s].max() <= 1e-9 and df[safe_f].max() <= 1e-9


def test_isolated_and_coincident_points():
    one = FO.fpfh([[0.1, -0.2, 0.3]], [[0.0, 0.0, 1.0]], 0.1)
    assert one["k"][0] == 0 and not one["spfh"].any() and not one["fpfh"].any() and not one["unsafe_fpfh"].any()
    # two coincident points: each the other's neighbour (k = 1), d == 0 bins nothing
    two = FO.fpfh([[0.1, -0.2, 0.3]] * 2, [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], 0.1)
    assert two["k"].tolist() == [1, 1] and not two["spfh"].any() and not two["fpfh"].any()
    # e parallel to n_a: |e x n_a| == 0 bins nothing either
    par = FO.fpfh([[0.0, 0.0, 0.0], [0.0, 0.0, 0.05]], [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], 0.1)
    assert par["k"].tolist() == [1, 1] and not par["spfh"].any()
    # a point far from the others of its fragment
    far = FO.fpfh([[0.0, 0.0, 0.0], [0.03, 0.0, 0.0], [5.0, 5.0, 5.0]], [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0],
                                                                        [1.0, 0.0, 0.0]], 0.1)
    assert far["k"].tolist() == [1, 1, 0] and not far["fpfh"][2].any() and far["spfh"][0].sum() == 300.0


def test_known_pair_feature():
    """x_j = x_i + (1, 0, 0) d, n_i = z, n_j = (sin 30, 0, cos 30): a1 = 0, a2 = 0.5 -> the roles swap:
    n_a = n_j, e = -x, f2 = -0.5; v = (e x n_a)/|.| = (0, cos 30, 0)/cos 30 = y; w = n_a x v = (-cos 30, 0, sin 30);
    f0 = atan2(w.z, n_a.z) = atan2(sin 30, cos 30) = 30 deg; f1 = v.n_b = 0"""
    s, c = 0.5, np.sqrt(0.75)
    r = FO.fpfh([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0]], [[0.0, 0.0, 1.0], [s, 0.0, c]], 0.1)
    want = np.zeros(33)
    want[int(np.floor(11 * (np.pi / 6 + np.pi) / (2 * np.pi)))] = 100.0      # bin 6
    want[11 + 5] = 100.0                                                      # f1 = 0: the middle bin
    want[22 + int(np.floor(11 * 0.25))] = 100.0                               # f2 = -0.5: bin 2
    np.testing.assert_array_equal(r["spfh"][0], want)
    assert not r["unsafe_spfh"][0]
    # the middle of bin 5 is no edge, an interior edge is: f1 = 1/11 sits on edge 6
    x = np.array([[5.5, 6.0, 0.0], [11.0, 6.0 + 2e-9, 10.999]])
    assert FO._near_edge(x).tolist() == [[False, True, False], [False, False, False]]


def test_small_shapes_leave_out_none():
    """the random-point fragments of the GPU test: no unsafe row at either radius (seed 0 is the first tried)"""
    frags, normals = FO.small_case()
    assert tuple(len(f) for f in frags) == FO.SMALL_SIZES
    assert (frags[6][-1] == frags[6][-2]).all()                                # the coincident pair
    on_face = [np.isclose(f / FO.SMALL_R_INDEX, np.round(f / FO.SMALL_R_INDEX), atol=1e-12).any(1).mean()
               for f in frags[4:]]
    assert min(on_face) > 0.2 and all((f < 0).any() and (f > 0).any() for f in frags[2:])
    for radius in FO.SMALL_RADII:
        res = FO.fpfh_batch(frags, normals, radius)
        print("small shapes, radius %g: k up to %s, unsafe %d" % (
            radius, [int(r["k"].max()) if len(r["k"]) else 0 for r in res], sum(int(r["unsafe_fpfh"].sum())
                                                                                for r in res)))
        assert not any(r["unsafe_fpfh"].any() or r["unsafe_spfh"].any() for r in res)
        assert res[6]["k"][-1] >= 1 and res[7]["k"].max() >= 3


def test_nearest_feature_ties_and_empty_target():
    F = np.array([[0.0, 1.0], [2.0, 2.0], [0.0, 1.0], [5.0, 5.0]])
    d, i = FO.nearest_feature(np.array([[0.0, 1.1], [4.0, 4.0]]), F)
    assert i.tolist() == [0, 3] and np.allclose(d, [0.01, 2.0])
    d, i = FO.nearest_feature(F[:2], F[:0])
    assert i.tolist() == [-1, -1] and np.isinf(d).all()


# ------------------------------------------------------------------------------------------------- Python surface
def _fake_fo(normals="absent", M=10, r=0.075):
    import torch
    fo = types.SimpleNamespace(r=r, M=M, B=1, xyz=torch.zeros(M, 3, dtype=torch.float64), normals=None, fpfh=None)
    if not isinstance(normals, str):
        fo.normals = normals
    return fo


def test_compute_fpfh_argument_errors():
    import torch
    from lib.overlap import FragmentOverlap
    with pytest.raises(ValueError, match="needs fo.normals"):
        FragmentOverlap.compute_fpfh(_fake_fo())
    for radius in (0.0, -1.0, 0.0751, float("nan")):
        with pytest.raises(ValueError, match="must lie in"):
            FragmentOverlap.compute_fpfh(_fake_fo(torch.zeros(10, 3, dtype=torch.float64)), radius)
    for bad in (torch.zeros(10, 3), torch.zeros(9, 3, dtype=torch.float64), np.zeros((10, 3)),
                torch.zeros(3, 10, dtype=torch.float64).t()):
        with pytest.raises(ValueError, match="contiguous fp64"):
            FragmentOverlap.compute_fpfh(_fake_fo(bad))


def test_match_and_register_argument_errors():
    import torch
    from lib.fpfh import feat_match, match_features, register_fpfh
    with pytest.raises(ValueError, match="channels"):
        match_features(torch.zeros(4, 65), [0, 4], [[0, 0]])
    with pytest.raises(ValueError, match="channels"):
        feat_match(torch.zeros(4, 0), [0, 4], [[0, 0]])
    with pytest.raises(ValueError, match="fp32"):
        match_features(torch.zeros(4, 33, dtype=torch.float64), [0, 4], [[0, 0]])
    with pytest.raises(ValueError, match="prefix sums"):
        match_features(torch.zeros(4, 33), [0, 5], [[0, 0]])
    with pytest.raises(ValueError, match="outside"):
        match_features(torch.zeros(4, 33), [0, 4], [[0, 1]])
    with pytest.raises(ValueError, match="needs fo.fpfh"):
        register_fpfh(_fake_fo(), [[0, 0]])
    assert match_features(torch.zeros(4, 33), [0, 4], np.zeros((0, 2))) == []


# ------------------------------------------------------------------------------------------------------------- ABI
@needs_lib
def test_fpfh_entry_point_validation():
    """mvr_compute_fpfh: scalars first, then the empty call, then the pointers (all before any HIP call)"""
    from lib import _native as N
    L = N.lib()
    Z = None
    one = 1   # any non-NULL address: no pointer is dereferenced before the checks have passed

    def call(index=Z, ib=0, xyz=Z, nrm=Z, off=Z, B=2, M=0, r=0.1, radius=0.1, fpfh=Z, spfh=Z, ws=Z, wb=0):
        return L.mvr_compute_fpfh(index, ib, xyz, nrm, off, B, M, r, radius, fpfh, spfh, ws, wb, Z)

    assert L.mvr_compute_fpfh_workspace_bytes(0) > 0
    assert L.mvr_compute_fpfh_workspace_bytes(1000) >= 1000 * 33 * 8
    assert call() == 0                                                   # M == 0: NULL pointers allowed
    for kw in ({"M": -1}, {"M": 2 ** 31}, {"B": 0}, {"B": 32768}, {"radius": 0.0}, {"radius": -1.0}, {"r": 0.0},
               {"radius": 0.11}, {"radius": float("nan")}, {"r": float("nan")}):
        assert call(**kw) == -1, kw                                      # scalars before the empty short-cut
    full = dict(index=one, ib=L.mvr_radius_index_bytes(10), xyz=one, nrm=one, off=one, M=10, fpfh=one, ws=one,
                wb=L.mvr_compute_fpfh_workspace_bytes(10))
    for name in ("index", "xyz", "nrm", "off", "fpfh", "ws"):
        assert call(**dict(full, **{name: Z})) == -1, name
    assert call(**dict(full, ib=full["ib"] - 1)) == -1
    assert call(**dict(full, wb=full["wb"] - 1)) == -1
    assert call(**dict(full, radius=0.2)) == -1                          # a scalar rule with every pointer there


@needs_lib
def test_feat_match_entry_point_validation():
    from lib import _native as N
    L = N.lib()
    Z, one = None, 1

    def call(F=Z, C=33, off=Z, B=2, M=0, pairs=Z, qoff=Z, P=0, nq=0, max_q=0, idx=Z, d2=Z):
        return L.mvr_feat_match(F, C, off, B, M, pairs, qoff, P, nq, max_q, idx, d2, Z)

    assert call() == 0                                                   # P == 0
    assert call(P=3) == 0                                                # pairs without queries
    assert call(nq=5, max_q=5) == 0                                      # P == 0 still
    for kw in ({"C": 0}, {"C": 65}, {"C": -1}, {"P": -1}, {"M": -1}, {"M": 2 ** 31}, {"nq": -1}, {"max_q": -1},
               {"max_q": 65535 * 256 + 1}, {"B": 0}, {"B": 32768}):
        assert call(**kw) == -1, kw
    full = dict(F=one, off=one, M=10, pairs=one, qoff=one, P=1, nq=5, max_q=5, idx=one)
    for name in ("F", "off", "pairs", "qoff", "idx"):
        assert call(**dict(full, **{name: Z})) == -1, name
    assert call(**dict(full, max_q=0)) == -1
    assert call(**dict(full, C=65)) == -1
    for C in (1, 64):
        assert call(C=C) == 0
