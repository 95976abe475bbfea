"""CPU-side checks of the generalized ICP: the oracle (tests/gicp_oracle.py) against ground truth and against the
point-to-plane oracle, the input conditions the GPU comparisons of test_gpu_gicp.py rest on (no correspondence, no
stopping test and no pivot test decided by rounding; the scheme and the helpers of test_icp_plane_host.py), the
Python surface's argument errors and the entry point's validation (returns before any HIP call)."""
import functools
import os
import types

import numpy as np
import pytest

from conftest import PKG
import icp_oracle as O
import icp_plane_oracle as PO
import gicp_oracle as GO
from test_icp_plane_host import MARGIN, _check_deltas, _check_margins

LIB = os.path.join(PKG, "libmvreg_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")


def _scene_normals():
    return [r["normals"] for r in PO.scene4_normals()]


def _err(results):
    poses = O.scene4()[1]
    return max(np.abs(r["T"] - O.gt_transform(poses, i, j)[:3]).max() for r, (i, j) in zip(results, O.SIX))


# ------------------------------------------------------------------------------------------------------ ground truth
def test_oracle_recovers_a_full_copy():
    """the target holds an exact copy of the source, so the residuals vanish at the true motion and Gauss-Newton
    closes in quadratically: 10 iterations from 1 degree / 5 mm reach the project's fp64 bound"""
    src = O.scene4_centroids()[0]
    tgt, Tt, Ts = O.full_copy_case(src)
    ns, nt = PO.estimate_normals(src, 0.075), PO.estimate_normals(tgt, 0.075)
    r = GO.gicp(src, tgt, ns["normals"], nt["normals"], Ts, 0.05, max_iters=10, tol_fitness=0.0, tol_rmse=0.0)
    print("full copy: |T - T_true| %.3g, rmse %.3g, cond(H) %.3g, trace %s"
          % (np.abs(r["T"] - Tt[:3]).max(), r["rmse"], max(r["cond"]), r["trace"][:6].tolist()))
    assert r["iters"] == 10 and r["status"] == 0 and r["n_corr"] == len(src) and r["fitness"] == 1.0
    np.testing.assert_allclose(r["T"], Tt[:3], rtol=0, atol=1e-9)
    _check_margins("full copy", [r])


def test_system_matches_a_per_correspondence_restatement():
    """gicp_oracle.system (batched einsum) against the sums written out one correspondence at a time"""
    rng = np.random.default_rng(0)
    k = 40
    q, y, c = rng.normal(0, 0.3, (k, 3)), rng.normal(0, 0.3, (k, 3)), rng.normal(0, 0.3, 3)
    n, m = (v / np.linalg.norm(v, axis=1, keepdims=True) for v in rng.standard_normal((2, k, 3)))
    H, g = GO.system(q, y, n, m, c, 1e-3)
    H2, g2 = np.zeros((6, 6)), np.zeros(6)
    for i in range(k):
        M = 2 * np.eye(3) - (1 - 1e-3) * (np.outer(n[i], n[i]) + np.outer(m[i], m[i]))
        w = q[i] - c
        G = np.concatenate([-np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]), np.eye(3)], 1)
        H2 += G.T @ np.linalg.inv(M) @ G
        g2 += G.T @ np.linalg.inv(M) @ (q[i] - y[i])
        ev = np.linalg.eigvalsh(M)
        assert 2e-3 * (1 - 1e-12) <= ev[0] and ev[2] <= 2 * (1 + 1e-12)
    assert np.abs(H - H2).max() <= 1e-9 * np.abs(H2).max() and np.abs(g - g2).max() <= 1e-9 * np.abs(g2).max()


# ------------------------------------------------------------------------------------ margins of the GPU test's cases
@functools.lru_cache(maxsize=None)
def _scene_runs():
    """the oracle on the scene cases of test_gpu_gicp.py (on the oracle's own centroids and normals: the same point
    sets in another row order, which moves the origin c and nothing the margins depend on)"""
    cent, nrm = O.scene4_centroids(), _scene_normals()
    T6 = O.scene4_starts(O.SIX, cent)
    run = lambda *a, **kw: GO.gicp_batch(cent, nrm, O.SIX, T6, *a, **kw)
    return {
        "30 iterations": run(0.075, 30, 0.0, 0.0),
        "30 iterations, max_dist 0.03": run(0.03, 30, 0.0, 0.0),
        "convergence": run(0.075, 30),
        "cap of 3": run(0.075, 3),
        "epsilon 1": run(0.075, 30, 0.0, 0.0, epsilon=1.0),
        "epsilon 1e-2": run(0.075, 30, 0.0, 0.0, epsilon=1e-2),
    }


@pytest.mark.parametrize("case", ["30 iterations", "30 iterations, max_dist 0.03", "convergence", "cap of 3",
                                  "epsilon 1", "epsilon 1e-2"])
def test_margins_of_the_scene_cases(case):
    res = _scene_runs()[case]
    _check_margins(case, res)
    _check_deltas(res)


def test_scene_statuses_and_error_below_point_to_plane():
    conv, cap = _scene_runs()["convergence"], _scene_runs()["cap of 3"]
    assert all(r["status"] == 0 and 0 < r["iters"] < 30 for r in conv), [(r["status"], r["iters"]) for r in conv]
    assert all(r["status"] == 2 and r["iters"] == 3 for r in cap)
    # what the feature buys: the error against ground truth after 30 fixed iterations, same starts
    cent = O.scene4_centroids()
    T6 = O.scene4_starts(O.SIX, cent)
    p2l = PO.icp_plane_batch(cent, _scene_normals(), O.SIX, T6, 0.075, 30, 0.0, 0.0)
    gen = _scene_runs()["30 iterations"]
    print("largest |T - T_gt| after 30 iterations: generalized %.3g, point-to-plane %.3g; iterations to converge %s"
          % (_err(gen), _err(p2l), [r["iters"] for r in conv]))
    assert _err(gen) < _err(p2l)


@functools.lru_cache(maxsize=None)
def _line_runs():
    frags, pairs, T0, _ = GO.line_case()
    nrm = [r["normals"] for r in PO.estimate_normals_batch(frags, PO.CORNER_RADIUS)]
    return {eps: GO.gicp_batch(frags, nrm, pairs, T0, GO.LINE_MAX_DIST, 30, 0.0, 0.0, epsilon=eps)
            for eps in (GO.EPSILON, 1.0)}


@pytest.mark.parametrize("epsilon", [GO.EPSILON, 1.0])
def test_margins_of_the_corner_and_line_case(epsilon):
    res = _line_runs()[epsilon]
    _check_margins("corner and line, epsilon %g" % epsilon, res)
    # the shapes do what the GPU test says of them: 0, 1, 5 points and the far source few correspondences; 6 points and
    # more a solve; the planar target is no degeneracy here (H holds sum M^-1); the line is one
    assert [r["status"] for r in res] == [1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 8]
    assert [r["n_corr"] for r in res][:4] == [0, 1, 5, 6] and res[8]["n_corr"] == 0
    assert [r["iters"] for r in res] == [0, 0, 0, 30, 30, 30, 30, 30, 0, 30, 0]
    assert res[10]["n_corr"] == 9 and len(res[10]["pivots"]) == 1


def test_margins_of_the_negated_and_shifted_scene_and_translation_invariance():
    """all normals negated: the oracle's sums hold only outer products, the same bits.  Every fragment moved by
    PO.SHIFT with conjugated starts: the margins of that run, and the oracle's own shifted / unshifted difference"""
    cent, nrm = O.scene4_centroids(), _scene_normals()
    T6 = O.scene4_starts(O.SIX, cent)
    ref = _scene_runs()["30 iterations"]
    neg = GO.gicp_batch(cent, [-n for n in nrm], O.SIX, T6, 0.075, 30, 0.0, 0.0)
    assert all(np.array_equal(a["T"], b["T"]) for a, b in zip(neg, ref))
    moved = [c + PO.SHIFT for c in cent]
    mn = [r["normals"] for r in PO.estimate_normals_batch(moved, PO.NORMAL_RADIUS)]
    res = GO.gicp_batch(moved, mn, O.SIX, PO.conjugate_starts(T6, PO.SHIFT), 0.075, 30, 0.0, 0.0)
    _check_margins("shifted scene", res)
    back = PO.conjugate_starts(np.asarray([np.concatenate([r["T"], [[0, 0, 0, 1.0]]]) for r in res]), -PO.SHIFT)
    diff = max(np.abs(back[k][:3] - ref[k]["T"]).max() for k in range(6))
    print("oracle, shifted by %s and conjugated back against unshifted: %.3g" % (PO.SHIFT.tolist(), diff))
    assert [r["n_corr"] for r in res] == [r["n_corr"] for r in ref]
    assert diff <= 1e-9


def test_margins_of_the_pair_case():
    """gicp_pair(normal_radius=0.09) on icp_oracle.pair_case()"""
    src, tgt, T0, max_dist, iters = O.pair_case()
    ns, nt = PO.estimate_normals(src, 0.09), PO.estimate_normals(tgt, 0.09)
    r = GO.gicp(src, tgt, ns["normals"], nt["normals"], T0, max_dist, iters)
    _check_margins("gicp_pair case", [r])
    _check_deltas([r])
    assert min(ns["edge"].min(), nt["edge"].min()) >= MARGIN and r["status"] in (0, 2)


def test_epsilon_one_does_not_depend_on_the_normals():
    cent = O.scene4_centroids()
    T6 = O.scene4_starts(O.SIX, cent)
    rng = np.random.default_rng(11)
    rnd = [rng.standard_normal(c.shape) for c in cent]
    rnd = [v / np.linalg.norm(v, axis=1, keepdims=True) for v in rnd]
    a = _scene_runs()["epsilon 1"]
    b = GO.gicp_batch(cent, rnd, O.SIX, T6, 0.075, 30, 0.0, 0.0, epsilon=1.0)
    diff = max(np.abs(x["T"] - y["T"]).max() for x, y in zip(a, b))
    print("epsilon 1, estimated against random unit normals: |dT| %.3g" % diff)
    assert diff <= 1e-12 and [x["n_corr"] for x in a] == [y["n_corr"] for y in b]
    # and with the normals in play the result is another one
    assert max(np.abs(x["T"] - y["T"]).max() for x, y in zip(a, _scene_runs()["30 iterations"])) > 1e-6


# --------------------------------------------------------------------------------------------------- Python surface
def test_gicp_argument_errors():
    import torch
    from lib.icp import gicp_refine, gicp_pair, METHODS
    assert METHODS == ("point_to_point", "point_to_plane")
    T = np.tile(np.eye(4), (2, 1, 1))
    pairs = [[0, 1], [1, 0]]
    fo = types.SimpleNamespace(r=0.075)      # every error below is raised before the index is touched
    with pytest.raises(ValueError, match="normals"):
        gicp_refine(fo, pairs, T)                                                 # no normals
    fo = types.SimpleNamespace(r=0.075, M=10, xyz=torch.zeros(10, 3, dtype=torch.float64))
    for bad in (None, np.zeros((10, 3)), torch.zeros(10, 3), torch.zeros(9, 3, dtype=torch.float64),
                torch.zeros(3, 10, dtype=torch.float64).t()):
        fo.normals = bad
        with pytest.raises(ValueError, match="normals"):
            gicp_refine(fo, pairs, T)
    fo.normals = torch.zeros(10, 3, dtype=torch.float64)
    for kw in (dict(epsilon=0.0), dict(epsilon=1.5), dict(epsilon=float("nan")), dict(epsilon=-1e-3)):
        with pytest.raises(ValueError, match="epsilon"):
            gicp_refine(fo, pairs, T, **kw)
    for kw in (dict(max_dist=0.08), dict(max_dist=0.0), dict(max_iters=-1), dict(tol_rmse=-1e-6),
               dict(tol_fitness=-1e-6)):
        with pytest.raises(ValueError):
            gicp_refine(fo, pairs, T, **kw)
    for bad_T, bad_pairs in ((T[0], pairs), (T.astype(np.int64), pairs), (T, pairs[:1]), (T, [0, 1])):
        with pytest.raises(ValueError):
            gicp_refine(fo, bad_pairs, bad_T)
    a, b = np.zeros((10, 3)), np.zeros((12, 3))
    for kw in (dict(epsilon=0.0), dict(epsilon=1.5), dict(epsilon=float("nan")), dict(normal_radius=0.0),
               dict(normal_radius=-1.0), dict(max_dist=0.0), dict(voxel_size=0.0), dict(max_iters=-1)):
        with pytest.raises(ValueError):
            gicp_pair(a, b, np.eye(4), **kw)
    with pytest.raises(ValueError):
        gicp_pair(a[:, :2], b, np.eye(4))
    with pytest.raises(ValueError):
        gicp_pair(a, b, np.eye(3))


# ------------------------------------------------------------------------------------------ the entry point's checks
def _gicp(L, P=1, M=10, B=2, r=0.075, max_dist=0.05, eps=1e-3, iters=30, tf=1e-6, tr=1e-6, ptrs=8, index=8,
          index_bytes=None, T=8, normals=8):
    """mvr_icp_refine_generalized with fake non-NULL device pointers (never dereferenced: every call here returns
    first)"""
    p = ptrs if ptrs else None
    ib = L.mvr_radius_index_bytes(max(M, 0)) if index_bytes is None else index_bytes
    return L.mvr_icp_refine_generalized(index if index else None, ib, p, normals if normals else None, p, B, M, r, p,
                                        p, P, max_dist, eps, iters, tf, tr, T if T else None, p, p, None, None, p,
                                        None, None)


@needs_lib
def test_entry_point_validation():
    from lib import _native
    L = _native.lib()
    # P = 0: MVR_OK before any pointer is read
    assert L.mvr_icp_refine_generalized(None, 0, None, None, None, 2, 0, 0.075, None, None, 0, 0.05, 1e-3, 30, 1e-6,
                                        1e-6, None, None, None, None, None, None, None, None) == 0
    assert _gicp(L, P=0, ptrs=0, index=0, T=0, normals=0) == 0
    assert _gicp(L, P=0, ptrs=0, index=0, T=0, normals=0, eps=1.0) == 0           # epsilon 1 is inside the range
    for bad in (dict(eps=0.0), dict(eps=1.5), dict(eps=float("nan")), dict(eps=-1e-3), dict(max_dist=0.08),
                dict(P=-1), dict(M=-1), dict(iters=-1), dict(B=0), dict(B=-3), dict(B=1 << 15), dict(max_dist=0.0),
                dict(max_dist=-0.05), dict(r=0.0), dict(r=-1.0), dict(tf=-1e-9), dict(tr=-1e-9),
                dict(max_dist=float("nan"))):
        assert _gicp(L, **bad) == -1, bad
        assert _gicp(L, P=0, **{k: v for k, v in bad.items() if k != "P"}) == (0 if "P" in bad else -1), bad
    assert _gicp(L, ptrs=0) == -1                      # NULL pairs / T0 / fitness / rmse / status
    assert _gicp(L, T=0) == -1                         # NULL T
    assert _gicp(L, index=0) == -1                     # NULL index with M > 0
    assert _gicp(L, normals=0) == -1                   # NULL normals with M > 0
    assert _gicp(L, index_bytes=L.mvr_radius_index_bytes(10) - 1) == -1   # a short index
