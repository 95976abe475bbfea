"""CPU-side checks of the coloured ICP: the oracle (tests/colored_icp_oracle.py) against ground truth and against
numpy's own solver, the input conditions the GPU comparisons of test_gpu_colored_icp.py rest on (no neighbour, no
correspondence, no stopping test and no pivot test decided by rounding), the Python surface's argument errors, the
entry points' validation (returns before any HIP call), the PLY colours and the CLI's parser."""
import functools
import os
import types

import numpy as np
import pytest

from conftest import PKG
import colored_icp_oracle as CO
import icp_oracle as O
import icp_plane_oracle as PO
import icp_robust_oracle as RO

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
    print("%s: smallest NN gap %.3g, |d - max_dist| %.3g, pivot ratio %.3g (refused: %.3g); iters %s, status %s"
          % (what, gap, edge, good, bad, [r["iters"] for r in results], [r["status"] for r in results]))
    assert gap >= MARGIN and edge >= MARGIN and good >= PIVOT_OK and bad <= PIVOT_DEGENERATE


# ----------------------------------------------------------------------------------------------------------- solvers
def test_oracle_solvers_against_numpy():
    rng = np.random.default_rng(0)
    for _ in range(20):
        B = rng.standard_normal((9, 3))
        A, h = B.T @ B, rng.standard_normal(3)
        d, ratio = CO.cholesky3(A, h)
        assert ratio > 1e-6 and np.abs(d - np.linalg.solve(A, h)).max() <= 1e-10 * np.abs(d).max()
    assert CO.cholesky3(np.diag([1.0, 0.0, 1.0]), np.ones(3))[0] is None            # a zero pivot
    assert CO.cholesky3(np.diag([1.0, 1e-13, 1.0]), np.ones(3))[0] is None          # below the floor
    assert CO.cholesky3(np.diag([1.0, np.nan, 1.0]), np.ones(3))[0] is None         # a NaN fails the test
    # the 6 x 6 system of a scene pair: icp_plane_oracle's Cholesky against np.linalg.solve
    cent, nrm, I, G = CO.scene4_inputs()
    T = O.scene4_starts(O.SIX, cent)[0][:3]
    st = O.evaluate(cent[0], cent[1], T, 0.075)
    H, b, w_sum = CO._system(cent[0], cent[1], nrm[1], I[0], I[1], G[1], T, st, cent[1][0], CO.LAMBDA, "l2", None)
    xi, ratio = PO.cholesky_solve(H, b)
    print("6 x 6 solve: pivot ratio %.3g, |xi - solve| %.3g" % (ratio, np.abs(xi + np.linalg.solve(H, b)).max()))
    assert np.abs(xi + np.linalg.solve(H, b)).max() <= 1e-12 and abs(w_sum - st["n_corr"]) <= 1e-9 * st["n_corr"]
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()


def test_lambda_one_is_the_plane_oracle():
    cent, nrm, I, G = CO.scene4_inputs()
    T0 = O.scene4_starts(O.SIX, cent)[0]
    a = CO.colored_icp(cent[0], cent[1], nrm[1], I[0], I[1], G[1], T0, 0.075, 1.0, max_iters=10, tol_fitness=0.0,
                       tol_rmse=0.0)
    b = PO.icp_plane(cent[0], cent[1], nrm[1], T0, 0.075, 10, 0.0, 0.0)
    assert np.abs(a["T"] - b["T"]).max() <= 1e-12 and a["n_corr"] == b["n_corr"]


# ------------------------------------------------------------------------------------ margins of the GPU test's cases
@pytest.mark.parametrize("radius", [0.075, 0.05])
def test_margins_of_the_scene_gradients(radius):
    cent, col = CO.scene4_colored_centroids()
    assert [len(c) for c in cent] == [len(c) for c in O.scene4_centroids()]
    assert all(2270 <= len(c) <= 2687 for c in cent)
    nrm = [r["normals"] for r in PO.estimate_normals_batch(cent, radius)]
    res = CO.color_gradients_batch(cent, nrm, col, radius)
    n_nbr = np.concatenate([r["n_nbr"] for r in res])
    piv = np.concatenate([r["pivot"] for r in res])
    edge = min(r["edge"].min() for r in res)
    print("radius %g: neighbours %d..%d, smallest pivot ratio %.3g, %d near the floor, smallest |d - radius| %.3g, "
          "largest gradient %.3g" % (radius, n_nbr.min(), n_nbr.max(), piv.min(), int(CO.near_floor(piv).sum()), edge,
                                     max(np.abs(r["grad"]).max() for r in res)))
    assert edge >= MARGIN and n_nbr.min() >= 4 and not CO.near_floor(piv).any() and piv.min() > 1e-7
    if radius == 0.075:
        assert n_nbr.min() >= 14 and piv.min() > 1e-6


@functools.lru_cache(maxsize=None)
def _scene_runs():
    """the oracle on the scene cases of test_gpu_colored_icp.py (on the oracle's own normals and gradients: the GPU's
    differ by rounding, which moves nothing the margins depend on)"""
    cent, nrm, I, G = CO.scene4_inputs()
    T6 = O.scene4_starts(O.SIX, cent)
    run = lambda *a, **kw: CO.colored_icp_batch(cent, nrm, I, G, O.SIX, T6, *a, **kw)
    out = {
        "30 iterations": run(0.075, max_iters=30, tol_fitness=0.0, tol_rmse=0.0),
        "30 iterations, max_dist 0.03": run(0.03, max_iters=30, tol_fitness=0.0, tol_rmse=0.0),
        "convergence": run(0.075),
        "cap of 3": run(0.075, max_iters=3),
        "lambda 1": run(0.075, 1.0, max_iters=30, tol_fitness=0.0, tol_rmse=0.0),
        "lambda 0.9": run(0.075, 0.9),
    }
    for kernel in RO.KERNELS[1:]:
        out[kernel] = run(0.075, CO.LAMBDA, kernel, CO.ROBUST_K, max_iters=3, tol_fitness=0.0, tol_rmse=0.0)
    return out


@pytest.mark.parametrize("case", ["30 iterations", "30 iterations, max_dist 0.03", "convergence", "cap of 3",
                                  "lambda 1", "lambda 0.9"] + list(RO.KERNELS[1:]))
def test_margins_of_the_scene_cases(case):
    res = _scene_runs()[case]
    _check_margins(case, res)
    _check_deltas(res)
    if case.startswith("30") or case == "lambda 1":
        assert all(r["iters"] == 30 and r["status"] == 0 for r in res)
    if case == "30 iterations":
        assert min(min(r["pivots"]) for r in res) >= 1e-3
    if case == "convergence":
        assert all(r["status"] == 0 and 0 < r["iters"] < 30 for r in res)
    if case == "cap of 3":
        assert all(r["status"] == 2 and r["iters"] == 3 for r in res)
    if case in RO.KERNELS:
        assert all(r["iters"] == 3 and r["status"] == 0 and r["w_sum"] > 0 for r in res)


def test_margins_of_the_small_colored_case():
    frags, colors = CO.small_colored_case()
    assert tuple(len(f) for f in frags) == PO.SMALL_SIZES + (4, 64)
    nb, row = CO.SMALL_NAN
    assert np.isnan(colors[nb][row]).any() and sum(int(np.isnan(c).sum()) for c in colors) == 1
    nrm = [r["normals"] for r in PO.estimate_normals_batch(frags, PO.SMALL_R_INDEX)]
    for radius in (PO.SMALL_R_INDEX, 0.06):
        res = CO.color_gradients_batch(frags, nrm, colors, radius)
        edge = min([r["edge"].min() for r in res if len(r["edge"])])
        piv = np.concatenate([r["pivot"] for r in res])
        ok = piv[np.isfinite(piv) & (piv > CO.PIVOT_FLOOR)]
        print("radius %g: smallest |d - radius| %.3g, %d of %d points near the floor, smallest pivot ratio of a solve "
              "%.3g, collinear fragment's largest %.3g" % (radius, edge, int(CO.near_floor(piv).sum()), len(piv),
                                                           ok.min(), res[CO.SMALL_LINE]["pivot"].max()))
        assert edge >= MARGIN and CO.near_floor(piv).mean() <= 0.05
        assert (res[CO.SMALL_FOUR]["n_nbr"] == 4).all() and (res[CO.SMALL_LINE]["n_nbr"] >= 4).all()
        assert (res[CO.SMALL_LINE]["pivot"] < CO.PIVOT_FLOOR / 10.0).all() and not res[CO.SMALL_LINE]["grad"].any()
        for b in (1, 2, 3):
            assert (res[b]["n_nbr"] < 4).all() and not res[b]["grad"].any()
        holds = res[nb]["nan"]
        assert holds[row] and 1 < holds.sum() < len(holds) and not res[nb]["grad"][holds].any()
        assert np.isfinite(np.concatenate([r["grad"] for r in res])).all()


def test_margins_of_the_corner_case():
    frags, pairs, T0 = PO.corner_case()
    colors = CO.corner_colors(frags)
    nrm = [r["normals"] for r in PO.estimate_normals_batch(frags, PO.CORNER_RADIUS)]
    gr = CO.color_gradients_batch(frags, nrm, colors, PO.CORNER_RADIUS)
    assert min(r["edge"].min() for r in gr if len(r["edge"])) >= MARGIN
    assert not gr[1]["grad"].any()                                                 # the constant-colour plane
    res = CO.colored_icp_batch(frags, nrm, [g["intensity"] for g in gr], [g["grad"] for g in gr], pairs, T0,
                               PO.CORNER_RADIUS, max_iters=30, tol_fitness=0.0, tol_rmse=0.0)
    _check_margins("corner", res)
    status = [r["status"] for r in res]
    assert status == [1, 1, 1, 0, 0, 0, 0, 0, 1, 8], status
    assert [r["iters"] for r in res] == [0, 0, 0, 30, 30, 30, 30, 30, 0, 0]
    assert [r["n_corr"] for r in res][:4] == [0, 1, 5, 6] and res[9]["n_corr"] >= 6 and len(res[9]["pivots"]) == 1


def test_textured_plane_oracle():
    """what test_gpu_colored_icp.py's docstring quotes: the coloured loop lands 4.1e-5 from the truth (seed 1:
    6.3e-5), point-to-plane is refused at its first solve, point-to-point does not leave the start"""
    for seed in (0, 1):
        src, sc, tgt, tc, Tt = CO.textured_plane_case(seed)
        nrm = PO.estimate_normals(tgt, CO.PLANE_RADIUS)
        gr = CO.color_gradients(tgt, nrm["normals"], tc, CO.PLANE_RADIUS)
        r = CO.colored_icp(src, tgt, nrm["normals"], CO.intensity(sc), gr["intensity"], gr["grad"], np.eye(4),
                           CO.PLANE_RADIUS, max_iters=CO.PLANE_ITERS, tol_fitness=0.0, tol_rmse=0.0)
        p2l = PO.icp_plane(src, tgt, nrm["normals"], np.eye(4), CO.PLANE_RADIUS, CO.PLANE_ITERS, 0.0, 0.0)
        p2p = O.icp(src, tgt, np.eye(4), CO.PLANE_RADIUS, CO.PLANE_ITERS, 0.0, 0.0)
        err, e_p2p = CO.motion_error(r["T"], Tt, src), CO.motion_error(p2p["T"], Tt, src)
        print("seed %d: start %.3g away, coloured %.3g, point-to-plane status %d (pivot ratio %.3g), point-to-point "
              "%.3g; gradient pivots from %.3g, neighbours from %d"
              % (seed, CO.motion_error(np.eye(4), Tt, src), err, p2l["status"], p2l["pivots"][-1], e_p2p,
                 gr["pivot"].min(), gr["n_nbr"].min()))
        _check_margins("textured plane", [r])
        assert r["status"] == 0 and r["iters"] == CO.PLANE_ITERS and err < 1e-4
        assert p2l["status"] == 8 and p2l["iters"] == 0 and e_p2p >= 100.0 * err
        assert min(nrm["edge"].min(), gr["edge"].min()) >= MARGIN and not CO.near_floor(gr["pivot"]).any()
        assert gr["n_nbr"].min() >= 4


def test_margins_of_the_pair_case():
    """colored_icp_pair(normal_radius=0.09) on icp_oracle.pair_case() with the field's colours"""
    src, tgt, T0, max_dist, iters = O.pair_case()
    sc, tc = CO.scene4_raw_colors()[0][4::8], CO.scene4_raw_colors()[1][4::8]
    nrm = PO.estimate_normals(tgt, 0.09)
    gr = CO.color_gradients(tgt, nrm["normals"], tc, 0.09)
    r = CO.colored_icp(src, tgt, nrm["normals"], CO.intensity(sc), gr["intensity"], gr["grad"], T0, max_dist,
                       max_iters=iters)
    _check_margins("colored_icp_pair case", [r])
    _check_deltas([r])
    assert min(nrm["edge"].min(), gr["edge"].min()) >= MARGIN and not CO.near_floor(gr["pivot"]).any()
    assert r["status"] in (0, 2)


@pytest.mark.parametrize("tilted", [False, True])
def test_linear_field_oracle(tilted):
    """seen: 4.2e-15 on the plane z = 0.3; 1.9e-12 on the tilted one, where A's condition (pivot ratio 2e-5) costs
    five digits"""
    pts, n, colors, a = CO.linear_field_case(tilted)
    gr = CO.color_gradients(pts, np.tile(n, (len(pts), 1)), colors, 0.075)
    diff = np.abs(gr["grad"] - (a - (a @ n) * n)).max()
    print("linear field%s: neighbours %d..%d, pivot ratio from %.3g, largest |gradient - (a - (a . n) n)| %.3g"
          % (", tilted" if tilted else "", gr["n_nbr"].min(), gr["n_nbr"].max(), gr["pivot"].min(), diff))
    assert gr["n_nbr"].min() >= 4 and gr["edge"].min() >= MARGIN and gr["pivot"].min() > 1e-6
    assert diff <= (1e-9 if tilted else 1e-13)


def test_oracle_translation_invariance():
    """the oracle's own shifted / unshifted difference (the bound of the GPU test is 1e-7 unless 100 x this exceeds
    it)"""
    cent, nrm, I, G = CO.scene4_inputs()
    _, col = CO.scene4_colored_centroids()
    T6 = O.scene4_starts(O.SIX, cent)
    moved = [c + PO.SHIFT for c in cent]
    nrm_m = [r["normals"] for r in PO.estimate_normals_batch(moved, PO.NORMAL_RADIUS)]
    gr = CO.color_gradients_batch(moved, nrm_m, col, PO.NORMAL_RADIUS)
    res = CO.colored_icp_batch(moved, nrm_m, [g["intensity"] for g in gr], [g["grad"] for g in gr], O.SIX,
                               PO.conjugate_starts(T6, PO.SHIFT), 0.075, max_iters=30, tol_fitness=0.0, tol_rmse=0.0)
    ref = _scene_runs()["30 iterations"]
    back = PO.conjugate_starts(np.asarray([np.concatenate([r["T"], [[0, 0, 0, 1.0]]]) for r in res]), -PO.SHIFT)
    diff = max(np.abs(back[k][:3] - ref[k]["T"]).max() for k in range(6))
    print("oracle, shifted by %s and conjugated back against unshifted: %.3g" % (PO.SHIFT.tolist(), diff))
    assert [r["n_corr"] for r in res] == [r["n_corr"] for r in ref]
    assert diff <= 1e-9


# --------------------------------------------------------------------------------------------------- Python surface
def test_colored_icp_argument_errors():
    import torch
    from lib.icp import METHODS, colored_icp_pair, colored_icp_refine
    assert METHODS == ("point_to_point", "point_to_plane")
    T = np.tile(np.eye(4), (2, 1, 1))
    pairs = [[0, 1], [1, 0]]
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    fo = types.SimpleNamespace(r=0.075, M=10, xyz=z(10, 3))      # every error is raised before the index is touched
    for missing in ("normals", "intensity", "color_grad"):
        fo.normals, fo.intensity, fo.color_grad = z(10, 3), z(10), z(10, 3)
        setattr(fo, missing, None)
        with pytest.raises(ValueError, match=missing):
            colored_icp_refine(fo, pairs, T)
    for name, bad in (("intensity", z(10, 1)), ("intensity", torch.zeros(10)), ("intensity", np.zeros(10)),
                      ("color_grad", z(9, 3)), ("color_grad", z(3, 10).t()), ("normals", z(10))):
        fo.normals, fo.intensity, fo.color_grad = z(10, 3), z(10), z(10, 3)
        setattr(fo, name, bad)
        with pytest.raises(ValueError, match=name):
            colored_icp_refine(fo, pairs, T)
    fo.normals, fo.intensity, fo.color_grad = z(10, 3), z(10), z(10, 3)
    for kw in (dict(max_dist=0.08), dict(max_dist=0.0), dict(max_iters=-1), dict(tol_rmse=-1e-6),
               dict(lambda_geometric=-0.1), dict(lambda_geometric=1.1), dict(lambda_geometric=float("nan")),
               dict(kernel="l1"), dict(kernel="huber"), dict(kernel="huber", kernel_k=0.0), dict(kernel_k=0.1)):
        with pytest.raises(ValueError):
            colored_icp_refine(fo, pairs, T, **kw)
    a, b = np.zeros((10, 3)), np.zeros((12, 3))
    for kw in (dict(normal_radius=0.0), dict(max_dist=0.0), dict(lambda_geometric=2.0), dict(voxel_size=-1.0),
               dict(kernel="tukey")):
        with pytest.raises(ValueError):
            colored_icp_pair(a, a, b, b, np.eye(4), **kw)


def test_colors_argument_of_fragment_overlap_and_register_scene():
    import torch
    from lib import multiview as MV
    from lib.overlap import FragmentOverlap, _color_rows
    rows = _color_rows([np.full((2, 3), 255, np.uint8), torch.full((1, 3), 0.25)], [2, 1])
    assert [r.dtype for r in rows] == [torch.float64] * 2 and rows[0].tolist() == [[1.0] * 3] * 2
    assert rows[1].tolist() == [[0.25] * 3]
    for bad, n in (([np.zeros((2, 3))], [2, 1]), ([np.zeros((2, 3)), np.zeros((2, 3))], [2, 1]),
                   ([np.zeros((2, 4)), np.zeros((1, 3))], [2, 1]),
                   ([np.zeros((2, 3), np.int32), np.zeros((1, 3))], [2, 1])):
        with pytest.raises(ValueError, match="colors"):
            _color_rows(bad, n)
    fo = types.SimpleNamespace(r=0.075, M=4, colors=None, normals=None)
    for kw in (dict(radius=0.08), dict(radius=0.0), dict(radius=float("nan"))):
        with pytest.raises(ValueError, match="radius"):
            FragmentOverlap.compute_color_gradients(fo, **kw)
    with pytest.raises(ValueError, match="colors"):
        FragmentOverlap.compute_color_gradients(fo)
    assert "colored" in MV.ICP_METHODS
    with pytest.raises(ValueError, match="colors"):
        MV.register_scene([None, None], 0.025, method="colored")
    with pytest.raises(ValueError, match="colors"):
        MV.register_scene([None, None], 0.025, colors=[None])
    with pytest.raises(ValueError, match="lambda"):
        MV.register_scene([None, None], 0.025, method="colored", colors=[None, None], icp_lambda_geometric=1.5)


def test_point_tensor_check_through_its_four_callers():
    """lib.overlap._point_tensor behind compute_fpfh, compute_color_gradients, lib.icp._run and _check_colored: a wrong
    shape, a wrong dtype and a non-contiguous tensor raise with each caller's own wording, a missing one with its
    hint"""
    import re
    import torch
    from lib.icp import colored_icp_refine, icp_refine
    from lib.overlap import FragmentOverlap
    M, T, pairs = 10, np.tile(np.eye(4), (1, 1, 1)), [[0, 0]]
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    bads = (z(M - 1, 3), torch.zeros(M, 3), z(3, M).t())

    def fo(**kw):
        base = dict(r=0.075, M=M, B=1, xyz=z(M, 3), normals=z(M, 3), colors=z(M, 3), intensity=z(M),
                    color_grad=z(M, 3), fpfh=None)
        return types.SimpleNamespace(**dict(base, **kw))
    tail = " tensor on the device of fo.xyz"
    callers = (
        (lambda f: FragmentOverlap.compute_fpfh(f), "normals",
         "compute_fpfh: fo.normals must be a contiguous fp64 [10,3]" + tail,
         "compute_fpfh: needs fo.normals (call fo.estimate_normals(viewpoints=...))"),
        (lambda f: FragmentOverlap.compute_color_gradients(f), "normals",
         "compute_color_gradients: fo.normals must be a contiguous fp64 [10,3]" + tail,
         "compute_color_gradients: needs fo.normals (call fo.estimate_normals())"),
        (lambda f: FragmentOverlap.compute_color_gradients(f), "colors",
         "compute_color_gradients: fo.colors must be a contiguous fp64 [10,3]" + tail,
         "compute_color_gradients: needs fo.colors (build the FragmentOverlap with colors=...)"),
        (lambda f: icp_refine(f, pairs, T, method="point_to_plane"), "normals",
         "icp_refine: fo.normals must be a contiguous fp64 [10,3]" + tail,
         "icp_refine: method 'point_to_plane' needs fo.normals (call fo.estimate_normals())"),
        (lambda f: colored_icp_refine(f, pairs, T), "color_grad",
         "colored_icp_refine: fo.color_grad must be a contiguous fp64 [10, 3]" + tail,
         "colored_icp_refine: needs fo.color_grad (call fo.compute_color_gradients())"),
    )
    for call, what, wrong, missing in callers:
        for bad in bads:
            with pytest.raises(ValueError, match="^" + re.escape(wrong) + "$"):
                call(fo(**{what: bad}))
        with pytest.raises(ValueError, match="^" + re.escape(missing) + "$"):
            call(fo(**{what: None}))
    for bad in (z(M, 1), torch.zeros(M), z(2 * M)[::2]):
        with pytest.raises(ValueError, match="^" + re.escape("colored_icp_refine: fo.intensity must be a contiguous "
                                                             "fp64 [10]" + tail) + "$"):
            colored_icp_refine(fo(intensity=bad), pairs, T)


def test_ball_radius_is_one_rule():
    import re
    from lib.overlap import _ball_radius, _iss_arguments, _radius_outlier_arguments
    r = 0.075
    assert _ball_radius("f: radius", r, r) == r and _ball_radius("f: radius", 0.05, r) == 0.05
    for bad in (0.0, -0.01, float("nan"), r * (1.0 + 1e-6)):
        msg = "f: radius %g must lie in (0, 0.075], the index's cell size (build the FragmentOverlap with radius >= it)"
        with pytest.raises(ValueError, match="^" + re.escape(msg % bad) + "$"):
            _ball_radius("f: radius", bad, r)
        with pytest.raises(ValueError, match="^" + re.escape("radius_outliers: radius %g must lie in" % bad)):
            _radius_outlier_arguments(16, bad, r)
        with pytest.raises(ValueError, match="^" + re.escape("iss_keypoints: non_max_radius %r must lie in" % bad)):
            _iss_arguments(None, bad, 0.975, 0.975, 5, 1e-6, r)
    assert _radius_outlier_arguments(16, None, r) == (16, r) and _iss_arguments(r, None, 0.975, 0.975, 5, 0.0, r)[0] == r


# ----------------------------------------------------------------------------------------- the entry points' checks
def _colored(L, P=1, M=10, B=2, r=0.075, max_dist=0.05, lam=0.968, kernel=0, k=0.0, iters=30, tf=1e-6, tr=1e-6, ptrs=8,
             index=8, T=8, normals=8, intensity=8, grad=8, index_bytes=None):
    """mvr_icp_refine_colored with fake non-NULL device pointers (never dereferenced: every call here returns first)"""
    p = ptrs if ptrs else None
    ib = L.mvr_radius_index_bytes(max(M, 0)) if index_bytes is None else index_bytes
    return L.mvr_icp_refine_colored(index if index else None, ib, p, normals if normals else None,
                                    intensity if intensity else None, grad if grad else None, p, B, M, r, p, p, P,
                                    max_dist, lam, kernel, k, iters, tf, tr, T if T else None, p, p, None, None, p,
                                    None, None, None)


def _gradient(L, M=10, B=2, r=0.075, radius=0.05, ptrs=8, index=8, index_bytes=None, normals=8, colors=8, out=8):
    p = ptrs if ptrs else None
    ib = L.mvr_radius_index_bytes(max(M, 0)) if index_bytes is None else index_bytes
    o = out if out else None
    return L.mvr_color_gradient(index if index else None, ib, p, normals if normals else None,
                                colors if colors else None, p, B, M, r, radius, o, o, None, None)


@needs_lib
def test_entry_point_validation_of_the_coloured_loop():
    from lib import _native
    L = _native.lib()
    # P = 0: MVR_OK before any pointer is read
    assert L.mvr_icp_refine_colored(None, 0, None, None, None, None, None, 2, 0, 0.075, None, None, 0, 0.05, 0.968, 0,
                                    0.0, 30, 1e-6, 1e-6, None, None, None, None, None, None, None, None, None) == 0
    assert _colored(L, P=0, ptrs=0, index=0, T=0, normals=0, intensity=0, grad=0) == 0
    for bad in (dict(P=-1), dict(M=-1), dict(iters=-1), dict(B=0), dict(B=1 << 15), dict(max_dist=0.0),
                dict(r=0.0), dict(max_dist=0.08), dict(tf=-1e-9), dict(tr=-1e-9), dict(max_dist=float("nan")),
                dict(lam=-1e-9), dict(lam=1.0 + 1e-9), dict(lam=float("nan")), dict(kernel=-1), dict(kernel=5),
                dict(kernel=1, k=0.0), dict(kernel=4, k=-1.0), dict(kernel=2, k=float("nan"))):
        assert _colored(L, **bad) == -1, bad
        assert _colored(L, P=0, **{k: v for k, v in bad.items() if k != "P"}) == (0 if "P" in bad else -1), bad
    for ok in (dict(lam=0.0), dict(lam=1.0), dict(kernel=0, k=-1.0)):                # k is not looked at for L2
        assert _colored(L, P=0, **ok) == 0, ok
    assert _colored(L, ptrs=0) == -1                   # NULL pairs / T0 / fitness / rmse / status
    assert _colored(L, T=0) == -1
    assert _colored(L, index=0) == -1
    assert _colored(L, normals=0) == -1                # with M > 0
    assert _colored(L, intensity=0) == -1
    assert _colored(L, grad=0) == -1
    assert _colored(L, index_bytes=L.mvr_radius_index_bytes(10) - 1) == -1


@needs_lib
def test_entry_point_validation_of_the_gradients_and_voxel_colours():
    from lib import _native
    L = _native.lib()
    # M = 0: MVR_OK before any pointer is read
    assert L.mvr_color_gradient(None, 0, None, None, None, None, 2, 0, 0.075, 0.075, None, None, None, None) == 0
    assert _gradient(L, M=0, ptrs=0, index=0, normals=0, colors=0, out=0) == 0
    for bad in (dict(M=-1), dict(B=0), dict(B=-3), dict(B=1 << 15), dict(radius=0.0), dict(radius=-0.05),
                dict(r=0.0), dict(radius=0.08), dict(radius=float("nan")), dict(r=float("nan"))):
        assert _gradient(L, **bad) == -1, bad
        assert _gradient(L, M=0, **{k: v for k, v in bad.items() if k != "M"}) == (0 if "M" in bad else -1), bad
    assert _gradient(L, ptrs=0) == -1                  # NULL xyz / off
    assert _gradient(L, out=0) == -1                   # NULL intensity / grad
    assert _gradient(L, index=0) == -1
    assert _gradient(L, normals=0) == -1
    assert _gradient(L, colors=0) == -1
    assert _gradient(L, index_bytes=L.mvr_radius_index_bytes(10) - 1) == -1
    # the coloured voxel pass: its own two pointers, then mvr_voxel_centroids' checks
    ws = L.mvr_voxel_centroids_workspace_bytes(10)
    assert L.mvr_voxel_centroids_colored(8, 8, 2, 10, 0.025, 8, ws, None, 8, 8, 8, None) == -1
    assert L.mvr_voxel_centroids_colored(8, 8, 2, 10, 0.025, 8, ws, 8, 8, 8, None, None) == -1
    assert L.mvr_voxel_centroids_colored(8, 8, 2, 10, 0.0, 8, ws, 8, 8, 8, 8, None) == -1
    assert L.mvr_voxel_centroids_colored(8, 8, 2, 10, 0.025, 8, ws - 1, 8, 8, 8, 8, None) == -1
    assert L.mvr_voxel_centroids_colored(8, None, 2, 10, 0.025, 8, ws, 8, 8, 8, 8, None) == -1


# --------------------------------------------------------------------------------------------------------------- PLY
def test_ply_colours_round_trip(tmp_path):
    from lib.ply import read_ply_colors, read_ply_xyz, write_ply
    rng = np.random.default_rng(0)
    xyz = rng.standard_normal((7, 3)).astype(np.float32)
    nrm = rng.standard_normal((7, 3)).astype(np.float32)
    u8 = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    for name, normals, colors in (("a", nrm, u8), ("b", None, u8), ("c", None, u8 / 255.0)):
        path = str(tmp_path / (name + ".ply"))
        write_ply(path, xyz, normals, colors)
        got_xyz, got_c = read_ply_colors(path)
        assert got_xyz.tobytes() == xyz.tobytes() and got_c.dtype == np.float64
        assert got_c.tobytes() == (u8 / 255.0).tobytes() and read_ply_xyz(path).tobytes() == xyz.tobytes()
    head = open(str(tmp_path / "a.ply"), "rb").read().split(b"end_header\n")[0].decode()
    assert "property float nx" in head and head.rstrip().endswith("property uchar blue")
    # without colours: None, and the bytes of the file are what they were before colours existed
    for name, normals in (("d", None), ("e", nrm)):
        path = str(tmp_path / (name + ".ply"))
        write_ply(path, xyz, normals)
        props = "xyz" if normals is None else ("x", "y", "z", "nx", "ny", "nz")
        want = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\n%send_header\n"
                % "".join("property float %s\n" % p for p in props)).encode() + \
            (xyz if normals is None else np.concatenate([xyz, nrm], 1)).astype("<f4").tobytes()
        assert open(path, "rb").read() == want
        assert read_ply_colors(path)[1] is None and read_ply_colors(path)[0].tobytes() == xyz.tobytes()
    # float and ascii colours, picked by name among other properties
    path = str(tmp_path / "f.ply")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                "property float blue\nproperty float quality\nproperty float green\nproperty float red\nend_header\n"
                "1 2 3 0.75 9 0.5 0.25\n4 5 6 0 9 1 0.125\n")
    got_xyz, got_c = read_ply_colors(path)
    assert got_xyz.tolist() == [[1, 2, 3], [4, 5, 6]] and got_c.tolist() == [[0.25, 0.5, 0.75], [0.125, 1.0, 0.0]]
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "g.ply"), xyz, None, u8[:5])


# --------------------------------------------------------------------------------------------------------------- CLI
def test_register_scene_cli_takes_the_coloured_method(tmp_path):
    from lib import multiview as MV
    from lib.ply import write_ply
    from scripts import register_scene as S
    assert S.ICP_METHODS == MV.ICP_METHODS and S.ICP_METHODS[-1] == "colored"
    ap = S.parser()
    base = ["--fragments", "a.ply", "b.ply", "--out", "o"]
    a = S.check_args(ap, ap.parse_args(base + ["--icp_method", "colored"]))
    assert a.icp_method == "colored" and a.icp_lambda_geometric == 0.968
    a = S.check_args(ap, ap.parse_args(base + ["--icp_method", "colored", "--icp_lambda_geometric", "0.9"]))
    assert a.icp_lambda_geometric == 0.9
    assert S.check_args(ap, ap.parse_args(base)).icp_method == "point_to_point"
    for bad in (["--icp_lambda_geometric", "1.5"], ["--icp_lambda_geometric", "-0.1"], ["--icp_method", "coloured"]):
        with pytest.raises(SystemExit):
            S.check_args(ap, ap.parse_args(base + bad))
    # the fragments' colours: read by name, and a file without them is named
    xyz = np.random.default_rng(0).standard_normal((5, 3)).astype(np.float32)
    u8 = np.random.default_rng(1).integers(0, 256, (5, 3)).astype(np.uint8)
    with_c, without = str(tmp_path / "with.ply"), str(tmp_path / "without.ply")
    write_ply(with_c, xyz, None, u8)
    write_ply(without, xyz)
    frags, colors = S.read_colored_fragments([with_c, with_c])
    assert frags[1].tobytes() == xyz.tobytes() and colors[0].tobytes() == (u8 / 255.0).tobytes()
    with pytest.raises(ValueError, match="without.ply"):
        S.read_colored_fragments([with_c, without])
    with pytest.raises(ValueError, match="without.ply"):
        S.main(["--fragments", with_c, without, "--out", str(tmp_path / "o"), "--icp_method", "colored"])
