"""CPU-side checks of the ICP refinement: the oracle (tests/icp_oracle.py) against ground truth, the input
conditions the GPU comparisons of test_gpu_icp.py rest on (no discrete choice decided by rounding), the Python
surface's argument errors and the entry point's validation (returns before any HIP call)."""
import functools
import os
import types

import numpy as np
import pytest

from conftest import PKG
import icp_oracle as O

LIB = os.path.join(PKG, "libmvreg_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")

MARGIN = 1e-8


@pytest.mark.parametrize("max_dist", [0.025, 0.05])
def test_oracle_recovers_a_full_copy(max_dist):
    src = O.scene4_centroids()[0]
    tgt, Tt, Ts = O.full_copy_case(src)
    r = O.icp(src, tgt, Ts, max_dist, max_iters=10, tol_fitness=0.0, tol_rmse=0.0)
    assert r["iters"] == 10 and r["status"] == 0 and r["n_corr"] == len(src) and r["fitness"] == 1.0
    print("full copy, max_dist %g: |T - T_true| %.3g, rmse %.3g, trace %s"
          % (max_dist, np.abs(r["T"] - Tt[:3]).max(), r["rmse"], r["trace"][:6].tolist()))
    np.testing.assert_allclose(r["T"], Tt[:3], rtol=0, atol=1e-9)
    assert min(O.min_margins([r])) >= MARGIN


@functools.lru_cache(maxsize=None)
def _scene_runs():
    """the oracle on the scene cases of test_gpu_icp.py (on the oracle's own centroids: the same point sets in
    another row order, which the margins do not depend on)"""
    cent, raw = O.scene4_centroids(), O.scene4()[0]
    T6 = O.scene4_starts(O.SIX, cent)
    return {
        "eval centroids": O.icp_batch(cent, O.TWELVE, O.eval_starts(cent), 0.075, 0),
        "eval raw": O.icp_batch(raw, O.TWELVE, O.eval_starts(raw), 0.05, 0),
        "30 iterations": O.icp_batch(cent, O.SIX, T6, 0.075, 30, 0.0, 0.0),
        "30 iterations, max_dist 0.03": O.icp_batch(cent, O.SIX, T6, 0.03, 30, 0.0, 0.0),
        "convergence": O.icp_batch(cent, O.SIX, T6, 0.075, 30),
        "cap of 3": O.icp_batch(cent, O.SIX, T6, 0.075, 3),
    }


def test_scene_sizes():
    assert [len(c) for c in O.scene4_centroids()] == [2687, 2531, 2270, 2621]


@pytest.mark.parametrize("case", ["eval centroids", "eval raw", "30 iterations", "30 iterations, max_dist 0.03",
                                  "convergence", "cap of 3"])
def test_margins_of_the_scene_cases(case):
    gap, edge = O.min_margins(_scene_runs()[case])
    print("%s: smallest NN gap %.3g, smallest |d - max_dist| %.3g" % (case, gap, edge))
    assert gap >= MARGIN and edge >= MARGIN


def test_margins_of_the_small_case():
    frags, pairs, T0 = O.small_case()
    res = O.icp_batch(frags, pairs, T0, O.SMALL_MAX_DIST, 30, 0.0, 0.0)
    gap, edge = O.min_margins(res)
    print("small shapes: smallest NN gap %.3g, smallest |d - max_dist| %.3g; n_corr %s, status %s"
          % (gap, edge, [r["n_corr"] for r in res], [r["status"] for r in res]))
    assert gap >= MARGIN and edge >= MARGIN
    # the shapes do what the GPU test says of them
    assert [r["status"] for r in res] == [1, 1, 1, 0, 0, 0, 0, 0, 1]
    assert [r["n_corr"] for r in res][:4] == [0, 1, 2, 3] and res[-1]["n_corr"] == 0
    assert [r["iters"] for r in res] == [0, 0, 0, 30, 30, 30, 30, 30, 0]


def test_margins_of_the_pair_case():
    src, tgt, T0, max_dist, iters = O.pair_case()
    r = O.icp(src, tgt, T0, max_dist, iters)
    gap, edge = O.min_margins([r])
    print("icp_pair case: smallest NN gap %.3g, smallest |d - max_dist| %.3g, deltas %s" % (gap, edge, r["deltas"]))
    assert gap >= MARGIN and edge >= MARGIN and r["iters"] == iters
    for df, dr in r["deltas"]:
        for d in (df, dr):
            assert not (1e-6 * (1 - 1e-3) <= d <= 1e-6 * (1 + 1e-3)), (df, dr)


def test_stopping_evaluations_are_not_decided_by_rounding():
    """no |delta fitness| or |delta rmse| of the convergence cases lies within a factor 1 +- 1e-3 of its tolerance
    (checked at every evaluation, the stopping one and the one before among them)"""
    runs = _scene_runs()
    conv = runs["convergence"]
    print("iterations to convergence: %s, status %s" % ([r["iters"] for r in conv], [r["status"] for r in conv]))
    assert sum(r["status"] == 0 and 0 < r["iters"] < 30 for r in conv) >= 4
    assert all(r["status"] == 2 and r["iters"] == 30 for r in conv if r["status"])
    assert all(r["status"] == 2 and r["iters"] == 3 for r in runs["cap of 3"])
    for r in conv + runs["cap of 3"]:
        for df, dr in r["deltas"]:
            for d in (df, dr):
                assert not (1e-6 * (1 - 1e-3) <= d <= 1e-6 * (1 + 1e-3)), (df, dr)


# --------------------------------------------------------------------------------------------------- Python surface
def test_icp_refine_argument_errors():
    from lib.icp import icp_refine, STATUS_FEW_CORRESPONDENCES, STATUS_ITERATION_CAP, STATUS_INVALID_PAIR
    assert (STATUS_FEW_CORRESPONDENCES, STATUS_ITERATION_CAP, STATUS_INVALID_PAIR) == (1, 2, 4)
    fo = types.SimpleNamespace(r=0.075)      # every error below is raised before the index is touched
    T = np.tile(np.eye(4), (2, 1, 1))
    pairs = [[0, 1], [1, 0]]
    for kw in (dict(max_dist=0.08), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_iters=-1),
               dict(tol_fitness=-1e-6), dict(tol_rmse=-1e-6)):
        with pytest.raises(ValueError):
            icp_refine(fo, pairs, T, **kw)
    for bad_T in (np.eye(4), np.zeros((2, 4, 3)), np.zeros((2, 2, 4)), np.zeros((2, 4, 4), np.int64)):
        with pytest.raises(ValueError):
            icp_refine(fo, pairs, bad_T)
    for bad_pairs in ([[0, 1]], [0, 1, 1, 0], [[0, 1, 2], [1, 0, 2]]):
        with pytest.raises(ValueError):
            icp_refine(fo, bad_pairs, T)


def test_icp_pair_argument_errors():
    from lib.icp import icp_pair
    a, b = np.zeros((10, 3)), np.zeros((12, 3))
    for args, kw in (((a, b, np.eye(3)), {}), ((a.T, b, np.eye(4)), {}), ((a, b[:, :2], np.eye(4)), {}),
                     ((a, b, np.eye(4)), dict(max_dist=0.0)), ((a, b, np.eye(4)), dict(voxel_size=0.0)),
                     ((a, b, np.eye(4)), dict(max_iters=-2)), ((a, b, np.eye(4)), dict(tol_rmse=-1.0))):
        with pytest.raises(ValueError):
            icp_pair(*args, **kw)


# ------------------------------------------------------------------------------------------ the entry point's checks
def _call(L, P=1, M=10, B=2, r=0.075, max_dist=0.05, iters=30, tf=1e-6, tr=1e-6, ptrs=8, index=8, index_bytes=None,
          T=8):
    """mvr_icp_refine with fake non-NULL device pointers (never dereferenced: every call here returns first)"""
    p = ptrs if ptrs else None
    ib = L.mvr_radius_index_bytes(max(M, 0)) if index_bytes is None else index_bytes
    return L.mvr_icp_refine(index if index else None, ib, p, p, B, M, r, p, p, P, max_dist, iters, tf, tr,
                            T if T else None, p, p, None, None, p, None, None)


@needs_lib
def test_entry_point_validation():
    from lib import _native
    L = _native.lib()
    # P = 0: MVR_OK before any pointer is read
    assert L.mvr_icp_refine(None, 0, None, None, 2, 0, 0.075, None, None, 0, 0.05, 30, 1e-6, 1e-6, None, None, None,
                            None, None, None, None, None) == 0
    assert _call(L, P=0, ptrs=0, index=0, T=0) == 0
    for bad in (dict(P=-1), dict(M=-1), dict(iters=-1), dict(B=0), dict(B=-3), dict(max_dist=0.0),
                dict(max_dist=-0.05), dict(r=0.0), dict(r=-1.0), dict(max_dist=0.08), dict(tf=-1e-9),
                dict(tr=-1e-9), dict(max_dist=float("nan"))):
        assert _call(L, **bad) == -1, bad
        assert _call(L, P=0, **{k: v for k, v in bad.items() if k != "P"}) == (0 if "P" in bad else -1), bad
    assert _call(L, ptrs=0) == -1                      # NULL pairs / T0 / fitness / rmse / status
    assert _call(L, T=0) == -1                         # NULL T
    assert _call(L, index=0) == -1                     # NULL index with M > 0
    assert _call(L, index_bytes=L.mvr_radius_index_bytes(10) - 1) == -1   # a short index
