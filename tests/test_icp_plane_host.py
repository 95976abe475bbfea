"""CPU-side checks of the normal estimation and the point-to-plane ICP: the oracle (tests/icp_plane_oracle.py)
against ground truth, the input conditions the GPU comparisons of test_gpu_icp_plane.py rest on (no neighbour, no
correspondence, no stopping test and no pivot test decided by rounding), the Python surface's argument errors and the
two entry points' validation (returns before any HIP call)."""
import functools
import os
import types

import numpy as np
import pytest

from conftest import PKG
import icp_oracle as O
import icp_plane_oracle as PO

LIB = os.path.join(PKG, "libmvreg_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")

MARGIN = 1e-8
PIVOT_OK, PIVOT_DEGENERATE = 1e-9, 1e-15


def _check_deltas(results, tol=1e-6):
    for r in results:
        for df, dr in r["deltas"]:
            for d in (df, dr):
                assert not (tol * (1 - 1e-3) <= d <= tol * (1 + 1e-3)), (df, dr)


def _check_margins(what, results):
    gap, edge = O.min_margins(results)
    good, bad = PO.pivot_range(results)
    cond = max([c for r in results for c in r["cond"]] + [0.0])
    print("%s: smallest NN gap %.3g, |d - max_dist| %.3g, pivot ratio %.3g (refused: %.3g), largest cond(H) %.3g; "
          "iters %s, status %s" % (what, gap, edge, good, bad, cond, [r["iters"] for r in results],
                                   [r["status"] for r in results]))
    assert gap >= MARGIN and edge >= MARGIN and good >= PIVOT_OK and bad <= PIVOT_DEGENERATE


# ------------------------------------------------------------------------------------------------------ ground truth
def test_oracle_recovers_a_full_copy():
    """normals estimated on the target with its distractors; the numpy run reaches 5e-16 after 4 iterations"""
    src = O.scene4_centroids()[0]
    tgt, Tt, Ts = O.full_copy_case(src)
    nrm = PO.estimate_normals(tgt, 0.075)
    r = PO.icp_plane(src, tgt, nrm["normals"], Ts, 0.05, max_iters=10, tol_fitness=0.0, tol_rmse=0.0)
    print("full copy: |T - T_true| %.3g, rmse %.3g, cond(H) %.3g, trace %s"
          % (np.abs(r["T"] - Tt[:3]).max(), r["rmse"], max(r["cond"]), r["trace"][:6].tolist()))
    assert r["iters"] == 10 and r["status"] == 0 and r["n_corr"] == len(src) and r["fitness"] == 1.0
    np.testing.assert_allclose(r["T"], Tt[:3], rtol=0, atol=1e-9)
    _check_margins("full copy", [r])
    assert nrm["edge"].min() >= MARGIN


def test_cholesky_and_lstsq_loops_agree():
    cent, nrm = O.scene4_centroids(), PO.scene4_normals()
    T0 = O.scene4_starts(O.SIX, cent)[0]
    a = PO.icp_plane(cent[0], cent[1], nrm[1]["normals"], T0, 0.075, 30, 0.0, 0.0)
    b = PO.icp_plane(cent[0], cent[1], nrm[1]["normals"], T0, 0.075, 30, 0.0, 0.0, solver="lstsq")
    print("Cholesky against lstsq after 30 iterations: |dT| %.3g" % np.abs(a["T"] - b["T"]).max())
    assert np.abs(a["T"] - b["T"]).max() <= 1e-12 and a["n_corr"] == b["n_corr"]


# ------------------------------------------------------------------------------------ margins of the GPU test's cases
@pytest.mark.parametrize("radius", [0.075, 0.05])
def test_margins_of_the_scene_normals(radius):
    res = PO.scene4_normals(radius)
    n_nbr = np.concatenate([r["n_nbr"] for r in res])
    gap = np.concatenate([r["gap"] for r in res])
    edge = min(r["edge"].min() for r in res)
    print("radius %g: neighbours %d..%d, smallest relative eigen-gap %.3g (%d below 1e-4), smallest |d - radius| %.3g"
          % (radius, n_nbr.min(), n_nbr.max(), gap.min(), int((gap < 1e-4).sum()), edge))
    assert edge >= MARGIN and n_nbr.min() >= 3
    assert (gap < 1e-4).mean() <= 0.05
    if radius == 0.075:
        assert (n_nbr.min(), n_nbr.max()) == (14, 56) and gap.min() > 1e-3


@functools.lru_cache(maxsize=None)
def _scene_runs():
    """the oracle on the scene cases of test_gpu_icp_plane.py (on the oracle's own centroids and normals: the same
    point sets in another row order, which moves the origin c and nothing the margins depend on)"""
    cent = O.scene4_centroids()
    nrm = [r["normals"] for r in PO.scene4_normals()]
    T6 = O.scene4_starts(O.SIX, cent)
    return {
        "30 iterations": PO.icp_plane_batch(cent, nrm, O.SIX, T6, 0.075, 30, 0.0, 0.0),
        "30 iterations, max_dist 0.03": PO.icp_plane_batch(cent, nrm, O.SIX, T6, 0.03, 30, 0.0, 0.0),
        "convergence": PO.icp_plane_batch(cent, nrm, O.SIX, T6, 0.075, 30),
        "cap of 3": PO.icp_plane_batch(cent, nrm, O.SIX, T6, 0.075, 3),
    }


@pytest.mark.parametrize("case", ["30 iterations", "30 iterations, max_dist 0.03", "convergence", "cap of 3"])
def test_margins_of_the_scene_cases(case):
    res = _scene_runs()[case]
    _check_margins(case, res)
    _check_deltas(res)


def test_scene_convergence_has_both_statuses_and_beats_point_to_point():
    conv, cap = _scene_runs()["convergence"], _scene_runs()["cap of 3"]
    # statuses 0 and 2 both occur: every pair converges within the 30 (4 to 12 solves), none within the cap of 3
    assert all(r["status"] == 0 and 0 < r["iters"] < 30 for r in conv), [(r["status"], r["iters"]) for r in conv]
    assert all(r["status"] == 2 and r["iters"] == 3 for r in cap)
    # what the feature buys: the error against ground truth after 30 fixed iterations, both methods, same starts
    cent, poses = O.scene4_centroids(), O.scene4()[1]
    T6 = O.scene4_starts(O.SIX, cent)
    p2p = O.icp_batch(cent, O.SIX, T6, 0.075, 30, 0.0, 0.0)
    p2l = _scene_runs()["30 iterations"]
    for k, (i, j) in enumerate(O.SIX):
        gt = O.gt_transform(poses, i, j)[:3]
        print("pair (%d, %d): |T - T_gt| point-to-plane %.3g, point-to-point %.3g"
              % (i, j, np.abs(p2l[k]["T"] - gt).max(), np.abs(p2p[k]["T"] - gt).max()))
    err = lambda rs: max(np.abs(r["T"] - O.gt_transform(poses, i, j)[:3]).max() for r, (i, j) in zip(rs, O.SIX))
    assert err(p2l) < err(p2p)


def test_margins_of_the_small_normals_case():
    frags = PO.small_normals_case()
    cells = frags[-1] / PO.SMALL_R_INDEX
    assert (np.abs(cells - np.round(cells)) < 1e-12).any(1).sum() >= 341          # a third on cell faces
    assert all((f[:, :2].min(0) < 0).all() and (f[:, :2].max(0) > 0).all() for f in frags[2:] if len(f) > 3)
    assert (frags[PO.PLANAR][:, 2] == 0.0).all()
    for radius in (PO.SMALL_R_INDEX, 0.06):
        res = PO.estimate_normals_batch(frags, radius)
        edge = min([r["edge"].min() for r in res if len(r["edge"])])
        gap = np.concatenate([r["gap"] for r in res])
        n_nbr = [(int(r["n_nbr"].min()), int(r["n_nbr"].max())) for r in res if len(r["n_nbr"])]
        print("radius %g: neighbours per fragment %s, %d of %d points below the eigen-gap 1e-4, smallest |d - radius| "
              "%.3g" % (radius, n_nbr, int((gap < 1e-4).sum()), len(gap), edge))
        assert edge >= MARGIN and (gap < 1e-4).mean() <= 0.05
        assert n_nbr[0] == (1, 1) and n_nbr[1] == (2, 2) and n_nbr[2] == (3, 3)
        flat = res[PO.PLANAR]
        assert flat["gap"][flat["n_nbr"] >= 3].min() >= 1e-4                      # no near-collinear neighbourhood
        assert (flat["n_nbr"] >= 3).sum() >= 32 and (np.abs(flat["normals"]) == [0.0, 0.0, 1.0]).all()
        assert (np.concatenate([r["n_nbr"] for r in res]) < 3).any() or radius > 0.06


@functools.lru_cache(maxsize=None)
def _corner_run():
    frags, pairs, T0 = PO.corner_case()
    nrm = [r["normals"] for r in PO.estimate_normals_batch(frags, PO.CORNER_RADIUS)]
    return PO.icp_plane_batch(frags, nrm, pairs, T0, PO.CORNER_RADIUS, 30, 0.0, 0.0)


def test_margins_of_the_corner_case():
    frags, pairs, T0 = PO.corner_case()
    nrm = PO.estimate_normals_batch(frags[:2], PO.CORNER_RADIUS)
    assert min(r["edge"].min() for r in nrm) >= MARGIN
    assert (np.abs(nrm[1]["normals"]) == [0.0, 0.0, 1.0]).all()                   # the planar target
    res = _corner_run()
    _check_margins("corner", res)
    # the shapes do what the GPU test says of them
    assert [r["status"] for r in res] == [1, 1, 1, 0, 0, 0, 0, 0, 1, 8]
    assert [r["n_corr"] for r in res][:4] == [0, 1, 5, 6] and res[8]["n_corr"] == 0
    assert [r["iters"] for r in res] == [0, 0, 0, 30, 30, 30, 30, 30, 0, 0]
    assert res[9]["n_corr"] >= 6 and len(res[9]["pivots"]) == 1


def test_margins_of_the_pair_case():
    """icp_pair(method='point_to_plane', normal_radius=0.09) on icp_oracle.pair_case()"""
    src, tgt, T0, max_dist, iters = O.pair_case()
    nrm = PO.estimate_normals(tgt, 0.09)
    r = PO.icp_plane(src, tgt, nrm["normals"], T0, max_dist, iters)
    _check_margins("icp_pair case", [r])
    _check_deltas([r])
    print("icp_pair case: smallest |d - radius| %.3g, eigen-gap %.3g" % (nrm["edge"].min(), nrm["gap"].min()))
    assert nrm["edge"].min() >= MARGIN and nrm["gap"].min() >= 1e-4 and r["status"] in (0, 2)


def test_oracle_translation_invariance():
    """the oracle's own shifted / unshifted difference (the bound of the GPU test is 1e-7 unless 100 x this exceeds
    it; seen: 6.7e-14)"""
    cent = O.scene4_centroids()
    T6 = O.scene4_starts(O.SIX, cent)
    moved = [c + PO.SHIFT for c in cent]
    nrm = [r["normals"] for r in PO.estimate_normals_batch(moved, PO.NORMAL_RADIUS)]
    res = PO.icp_plane_batch(moved, nrm, O.SIX, PO.conjugate_starts(T6, PO.SHIFT), 0.075, 30, 0.0, 0.0)
    ref = _scene_runs()["30 iterations"]
    back = PO.conjugate_starts(np.asarray([np.concatenate([r["T"], [[0, 0, 0, 1.0]]]) for r in res]), -PO.SHIFT)
    diff = max(np.abs(back[k][:3] - ref[k]["T"]).max() for k in range(6))
    print("oracle, shifted by %s and conjugated back against unshifted: %.3g" % (PO.SHIFT.tolist(), diff))
    assert [r["n_corr"] for r in res] == [r["n_corr"] for r in ref]
    assert diff <= 1e-9


# --------------------------------------------------------------------------------------------------- Python surface
def test_icp_refine_plane_argument_errors():
    from lib.icp import icp_refine, icp_pair, STATUS_DEGENERATE, METHODS
    assert STATUS_DEGENERATE == 8 and METHODS == ("point_to_point", "point_to_plane")
    T = np.tile(np.eye(4), (2, 1, 1))
    pairs = [[0, 1], [1, 0]]
    fo = types.SimpleNamespace(r=0.075)      # every error below is raised before the index is touched
    with pytest.raises(ValueError):
        icp_refine(fo, pairs, T, method="plane")
    with pytest.raises(ValueError, match="normals"):
        icp_refine(fo, pairs, T, method="point_to_plane")                         # no normals
    import torch
    fo = types.SimpleNamespace(r=0.075, M=10, xyz=torch.zeros(10, 3, dtype=torch.float64))
    for bad in (None, np.zeros((10, 3)), torch.zeros(10, 3), torch.zeros(9, 3, dtype=torch.float64),
                torch.zeros(3, 10, dtype=torch.float64).t()):
        fo.normals = bad
        with pytest.raises(ValueError, match="normals"):
            icp_refine(fo, pairs, T, method="point_to_plane")
    fo.normals = torch.zeros(10, 3, dtype=torch.float64)
    for kw in (dict(max_dist=0.08), dict(max_iters=-1), dict(tol_rmse=-1e-6)):
        with pytest.raises(ValueError):
            icp_refine(fo, pairs, T, method="point_to_plane", **kw)
    a, b = np.zeros((10, 3)), np.zeros((12, 3))
    for kw in (dict(method="p2l"), dict(method="point_to_plane", normal_radius=0.0),
               dict(method="point_to_plane", normal_radius=-1.0), dict(method="point_to_plane", max_dist=0.0)):
        with pytest.raises(ValueError):
            icp_pair(a, b, np.eye(4), **kw)


def test_estimate_normals_argument_errors():
    from lib.overlap import FragmentOverlap
    fo = types.SimpleNamespace(r=0.075, B=2)
    for kw in (dict(radius=0.08), dict(radius=0.0), dict(radius=-0.05), dict(radius=float("nan")),
               dict(viewpoints=np.zeros((3, 3))), dict(viewpoints=np.zeros((2, 2))),
               dict(viewpoints=np.zeros((2, 3), np.int64))):
        with pytest.raises(ValueError):
            FragmentOverlap.estimate_normals(fo, **kw)


# ----------------------------------------------------------------------------------------- the entry points' checks
def _plane(L, P=1, M=10, B=2, r=0.075, max_dist=0.05, iters=30, tf=1e-6, tr=1e-6, ptrs=8, index=8, index_bytes=None,
           T=8, normals=8):
    """mvr_icp_refine_plane with fake non-NULL device pointers (never dereferenced: every call here returns first)"""
    p = ptrs if ptrs else None
    ib = L.mvr_radius_index_bytes(max(M, 0)) if index_bytes is None else index_bytes
    return L.mvr_icp_refine_plane(index if index else None, ib, p, normals if normals else None, p, B, M, r, p, p, P,
                                  max_dist, iters, tf, tr, T if T else None, p, p, None, None, p, None, None)


def _normals(L, M=10, B=2, r=0.075, radius=0.05, ptrs=8, index=8, index_bytes=None, out=8):
    p = ptrs if ptrs else None
    ib = L.mvr_radius_index_bytes(max(M, 0)) if index_bytes is None else index_bytes
    return L.mvr_estimate_normals(index if index else None, ib, p, p, B, M, r, radius, None, out if out else None,
                                  None, None)


@needs_lib
def test_entry_point_validation_of_the_plane_loop():
    from lib import _native
    L = _native.lib()
    # P = 0: MVR_OK before any pointer is read
    assert L.mvr_icp_refine_plane(None, 0, None, None, None, 2, 0, 0.075, None, None, 0, 0.05, 30, 1e-6, 1e-6, None,
                                  None, None, None, None, None, None, None) == 0
    assert _plane(L, P=0, ptrs=0, index=0, T=0, normals=0) == 0
    for bad in (dict(P=-1), dict(M=-1), dict(iters=-1), dict(B=0), dict(B=-3), dict(B=1 << 15), dict(max_dist=0.0),
                dict(max_dist=-0.05), dict(r=0.0), dict(r=-1.0), dict(max_dist=0.08), dict(tf=-1e-9),
                dict(tr=-1e-9), dict(max_dist=float("nan"))):
        assert _plane(L, **bad) == -1, bad
        assert _plane(L, P=0, **{k: v for k, v in bad.items() if k != "P"}) == (0 if "P" in bad else -1), bad
    assert _plane(L, ptrs=0) == -1                     # NULL pairs / T0 / fitness / rmse / status
    assert _plane(L, T=0) == -1                        # NULL T
    assert _plane(L, index=0) == -1                    # NULL index with M > 0
    assert _plane(L, normals=0) == -1                  # NULL normals with M > 0
    assert _plane(L, index_bytes=L.mvr_radius_index_bytes(10) - 1) == -1   # a short index


@needs_lib
def test_entry_point_validation_of_the_normals():
    from lib import _native
    L = _native.lib()
    # M = 0: MVR_OK before any pointer is read
    assert L.mvr_estimate_normals(None, 0, None, None, 2, 0, 0.075, 0.075, None, None, None, None) == 0
    assert _normals(L, M=0, ptrs=0, index=0, out=0) == 0
    for bad in (dict(M=-1), dict(B=0), dict(B=-3), dict(B=1 << 15), dict(radius=0.0), dict(radius=-0.05),
                dict(r=0.0), dict(r=-1.0), dict(radius=0.08), dict(radius=float("nan")), dict(r=float("nan"))):
        assert _normals(L, **bad) == -1, bad
        assert _normals(L, M=0, **{k: v for k, v in bad.items() if k != "M"}) == (0 if "M" in bad else -1), bad
    assert _normals(L, ptrs=0) == -1                   # NULL xyz / off
    assert _normals(L, out=0) == -1                    # NULL normals
    assert _normals(L, index=0) == -1                  # NULL index
    assert _normals(L, index_bytes=L.mvr_radius_index_bytes(10) - 1) == -1   # a short index
