"""CPU-side checks of the robust kernels on the ICP variants: the oracle (tests/icp_robust_oracle.py) against the three
plain oracles with 'l2', the weights at their corners, what the kernels buy on the contaminated case, the input
conditions the GPU comparisons of test_gpu_icp_robust.py rest on, the entry point's validation (returns before any HIP
call), the Python surface's argument errors and the command line's parsing."""
import functools
import os
import types

import numpy as np
import pytest

from conftest import PKG
import gicp_oracle as GO
import icp_oracle as O
import icp_plane_oracle as PO
import icp_robust_oracle as RO

LIB = os.path.join(PKG, "libmvreg_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")

# A discrete choice (which neighbour, inside max_dist or not) is the same in two fp64 computations when its margin
# exceeds twice their difference in q.  That difference is rounding, about 1e-13 over 30 solves (what the plain
# loops' GPU tests print); 1e-9, the parity tolerance itself, leaves four orders.  (The plain loops' cases keep 1e-8;
# Huber's point-to-point run on the scene passes one query with a gap of 4.7e-9.)
MARGIN = 1e-9
FLOATS = ("T", "fitness", "rmse", "trace")


# ------------------------------------------------------------------------------------- l2 is the three plain oracles
def _same(what, got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        for name in ("n_corr", "iters", "status"):
            assert g[name] == w[name], (what, k, name)
        diff = max(float(np.abs(np.asarray(g[name]) - np.asarray(w[name])).max()) for name in FLOATS)
        print("%s, pair %d: l2 against the plain oracle %.3g; w_sum %g, n_corr %d" % (what, k, diff, g["w_sum"],
                                                                                       g["n_corr"]))
        assert diff <= 1e-12 and g["w_sum"] == g["n_corr"]


def test_l2_is_the_point_to_point_oracle():
    cent = O.scene4_centroids()
    T6 = O.scene4_starts(O.SIX, cent)
    for iters, tol in ((30, 0.0), (30, 1e-6), (3, 1e-6)):
        _same("scene, %d / %g" % (iters, tol),
              RO.icp_robust_batch("point_to_point", cent, None, O.SIX, T6, 0.075, "l2", None, iters, tol, tol),
              O.icp_batch(cent, O.SIX, T6, 0.075, iters, tol, tol))
    frags, pairs, T0 = O.small_case()
    pairs = np.concatenate([pairs, [[len(frags), 0]]])                  # and an invalid pair
    T0 = np.concatenate([T0, T0[:1]])
    _same("small", RO.icp_robust_batch("point_to_point", frags, None, pairs, T0, O.SMALL_MAX_DIST, "l2", None, 30,
                                       0.0, 0.0), O.icp_batch(frags, pairs, T0, O.SMALL_MAX_DIST, 30, 0.0, 0.0))


def test_l2_is_the_point_to_plane_oracle():
    cent, nrm = O.scene4_centroids(), [r["normals"] for r in PO.scene4_normals()]
    T6 = O.scene4_starts(O.SIX, cent)
    for iters, tol in ((30, 0.0), (30, 1e-6)):
        _same("scene, %d / %g" % (iters, tol),
              RO.icp_robust_batch("point_to_plane", cent, nrm, O.SIX, T6, 0.075, "l2", None, iters, tol, tol),
              PO.icp_plane_batch(cent, nrm, O.SIX, T6, 0.075, iters, tol, tol))
    frags, pairs, T0 = PO.corner_case()
    nrm = [r["normals"] for r in PO.estimate_normals_batch(frags, PO.CORNER_RADIUS)]
    got = RO.icp_robust_batch("point_to_plane", frags, nrm, pairs, T0, PO.CORNER_RADIUS, "l2", None, 30, 0.0, 0.0)
    _same("corner", got, PO.icp_plane_batch(frags, nrm, pairs, T0, PO.CORNER_RADIUS, 30, 0.0, 0.0))
    assert got[-1]["status"] == 8 and got[-1]["w_sum"] == got[-1]["n_corr"] >= 6    # the planar target: w_sum is there


def test_l2_is_the_generalized_oracle():
    cent, nrm = O.scene4_centroids(), [r["normals"] for r in PO.scene4_normals()]
    T6 = O.scene4_starts(O.SIX, cent)
    for iters, tol, eps in ((30, 0.0, GO.EPSILON), (30, 1e-6, 1e-2)):
        _same("scene, %d / %g, epsilon %g" % (iters, tol, eps),
              RO.icp_robust_batch("generalized", cent, nrm, O.SIX, T6, 0.075, "l2", None, iters, tol, tol, eps),
              GO.gicp_batch(cent, nrm, O.SIX, T6, 0.075, iters, tol, tol, eps))
    frags, pairs, T0, _ = GO.line_case()
    nrm = [r["normals"] for r in PO.estimate_normals_batch(frags, PO.CORNER_RADIUS)]
    _same("line", RO.icp_robust_batch("generalized", frags, nrm, pairs, T0, GO.LINE_MAX_DIST, "l2", None, 30, 0.0, 0.0),
          GO.gicp_batch(frags, nrm, pairs, T0, GO.LINE_MAX_DIST, 30, 0.0, 0.0))


# ------------------------------------------------------------------------------------------------------- the weights
def test_weights_at_zero_at_k_and_beyond():
    k = 0.03
    r = np.array([0.0, 0.5 * k, -0.5 * k, k, -k, np.nextafter(k, 1.0), 2.0 * k, -2.0 * k, 1e3])
    np.testing.assert_array_equal(RO.weight("l2", None, r), np.ones(9))
    np.testing.assert_array_equal(RO.weight("huber", k, r),
                                  [1, 1, 1, 1, 1, k / np.nextafter(k, 1.0), 0.5, 0.5, k / 1e3])
    np.testing.assert_allclose(RO.weight("cauchy", k, r)[[0, 1, 3, 6]], [1.0, 0.8, 0.5, 0.2], rtol=1e-15)
    np.testing.assert_allclose(RO.weight("gm", k, r)[[0, 3]], [1.0 / k, k / (k + k * k) ** 2], rtol=1e-15)
    tukey = RO.weight("tukey", k, r)
    np.testing.assert_allclose(tukey[:3], [1.0, 0.5625, 0.5625], rtol=1e-15)
    np.testing.assert_array_equal(tukey[3:], np.zeros(6))               # continuous at |r| == k: exactly 0 from there
    for name in RO.KERNELS[1:]:                                          # even, at most w(0), never negative
        kk = k * k if name == "gm" else k
        w = RO.weight(name, kk, r)
        assert np.all(w >= 0) and np.all(w <= w[0]) and w[1] == w[2] and w[6] == w[7], name
        below, above = RO.weight(name, kk, np.array([np.nextafter(kk, 0.0), np.nextafter(kk, 1.0)]))
        assert abs(below - above) <= 1e-15 * max(w[0], 1.0), name       # no jump at |r| == k
    with pytest.raises(ValueError):
        RO.weight("l1", k, r)


def test_weighted_kabsch():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((50, 3))
    Tt = O.rigid([0.3, -1.0, 0.2], 40.0, [0.5, 0.1, -2.0])
    y = x @ Tt[:3, :3].T + Tt[:3, 3]
    y[:10] += rng.standard_normal((10, 3))                              # outliers, weight 0
    w = np.concatenate([np.zeros(10), rng.uniform(0.1, 2.0, 40)])
    np.testing.assert_allclose(RO.weighted_kabsch(x, y, w), Tt[:3], rtol=0, atol=1e-13)
    np.testing.assert_allclose(RO.weighted_kabsch(x, y, np.ones(50)), O.kabsch(x, y), rtol=0, atol=1e-14)
    assert RO.weighted_kabsch(x, y, np.zeros(50)) is None
    assert RO.weighted_kabsch(x, y, np.full(50, np.nan)) is None


# ------------------------------------------------------------------------------------------- the contaminated case
@functools.lru_cache(maxsize=None)
def _contaminated(method, kernel):
    src, tgt, Tt, T0 = RO.contaminated_case()
    ns = PO.estimate_normals(src, PO.CORNER_RADIUS)["normals"]
    nt = PO.estimate_normals(tgt, PO.CORNER_RADIUS)["normals"]
    k = RO.CONTAMINATED_K ** 2 if kernel == "gm" else RO.CONTAMINATED_K
    r = RO.icp_robust(method, src, tgt, ns, nt, T0, RO.CONTAMINATED_MAX_DIST, kernel, k, RO.CONTAMINATED_ITERS, 0.0,
                      0.0)
    return r, RO.motion_error(r["T"], Tt, tgt)


@pytest.mark.parametrize("method", RO.METHODS)
def test_tukey_at_least_halves_the_error_of_l2_on_the_contaminated_case(method):
    """30 % of the source displaced by 6 cm inside max_dist 0.1.  Measured on the oracle (mm, l2 / huber / cauchy /
    gm / tukey): point-to-point 12.8 / 10.2 / 4.96 / 2.03 / 0.363, point-to-plane 26.5 / 26.4 / 21.5 / 12.1 / 1.19,
    generalized 25.9 / 5.51 / 1.96 / 0.988 / 0.843: the generalized loop meets the factor too, so it is asserted."""
    err = {}
    for kernel in RO.KERNELS:
        r, err[kernel] = _contaminated(method, kernel)
        gap, edge = O.min_margins([r])
        assert r["iters"] == 30 and r["status"] == 0 and gap >= MARGIN and edge >= MARGIN, kernel
    print("%s: error in mm %s" % (method, {k: round(1e3 * v, 3) for k, v in err.items()}))
    assert err["tukey"] <= 0.5 * err["l2"]
    assert all(err[k] < err["l2"] for k in RO.KERNELS[1:])              # the others fall between
    r = _contaminated(method, "tukey")[0]
    assert 0.0 < r["w_sum"] < r["n_corr"] == 600                        # every point is matched, not every one counts


# ------------------------------------------------------------------------------- margins of the GPU test's scene cases
@pytest.mark.parametrize("method", RO.METHODS)
@pytest.mark.parametrize("kernel", RO.KERNELS[1:])
def test_margins_of_the_scene_cases(method, kernel):
    """no correspondence and no stopping test of test_gpu_icp_robust.py's parity runs is decided by rounding (on the
    oracle's own centroids and normals: the same point sets in another row order)"""
    cent, nrm = O.scene4_centroids(), [r["normals"] for r in PO.scene4_normals()]
    T6 = O.scene4_starts(O.SIX, cent)
    for iters in (30, 3):
        res = RO.icp_robust_batch(method, cent, nrm, O.SIX, T6, 0.075, kernel, RO.SCENE_K[kernel], iters)
        gap, edge = O.min_margins(res)
        print("%s, %s, cap %d: smallest NN gap %.3g, |d - max_dist| %.3g, iters %s, status %s"
              % (method, kernel, iters, gap, edge, [r["iters"] for r in res], [r["status"] for r in res]))
        assert gap >= MARGIN and edge >= MARGIN
        for r in res:
            assert r["status"] in (0, 2) and (r["status"] == 0 or r["iters"] == iters)
            for d in [x for pair in r["deltas"] for x in pair]:
                assert not (1e-6 * (1 - 1e-3) <= d <= 1e-6 * (1 + 1e-3)), d
            if method != "point_to_point":
                assert min(r["pivots"]) >= 1e-9
        if iters == 3:                                                  # the cap: nothing converges within 3 solves
            assert all(r["status"] == 2 and r["iters"] == 3 for r in res)
        elif (method, kernel) != ("point_to_point", "tukey"):           # the tolerances: some pair stops on them
            assert any(r["status"] == 0 and 0 < r["iters"] < 30 for r in res)
        else:   # Tukey's point-to-point loop still moves by more than 1e-6 per step after 30 solves, on every pair
            assert all(r["status"] == 2 for r in res)


# ------------------------------------------------------------------------------------------ the entry point's checks
def _robust(L, P=1, M=10, B=2, r=0.075, method=0, max_dist=0.05, eps=1e-3, kernel=4, k=0.03, iters=30, tf=1e-6,
            tr=1e-6, ptrs=8, index=8, index_bytes=None, T=8, normals=8, w_sum=8):
    """mvr_icp_refine_robust with fake non-NULL device pointers (never dereferenced: every call here returns first)"""
    p = ptrs if ptrs else None
    ib = L.mvr_radius_index_bytes(max(M, 0)) if index_bytes is None else index_bytes
    return L.mvr_icp_refine_robust(index if index else None, ib, p, normals if normals else None, p, B, M, r, p, p, P,
                                   method, max_dist, eps, kernel, k, iters, tf, tr, T if T else None, p, p, None, None,
                                   p, None, w_sum if w_sum else None, None)


@needs_lib
def test_entry_point_validation():
    from lib import _native
    L = _native.lib()
    # P = 0: MVR_OK before any pointer is read, for every method and kernel
    for method in range(3):
        for kernel in range(5):
            assert _robust(L, P=0, method=method, kernel=kernel, ptrs=0, index=0, T=0, normals=0, w_sum=0) == 0
    assert _robust(L, P=0, kernel=0, k=float("nan"), ptrs=0) == 0       # l2 does not look at kernel_k
    assert _robust(L, P=0, kernel=0, k=-1.0, ptrs=0) == 0
    assert _robust(L, P=0, method=0, eps=0.0) == 0 and _robust(L, P=0, method=1, eps=float("nan")) == 0   # nor these
    common = (dict(max_dist=0.08), dict(P=-1), dict(M=-1), dict(iters=-1), dict(B=0), dict(B=-3), dict(B=1 << 15),
              dict(max_dist=0.0), dict(max_dist=-0.05), dict(r=0.0), dict(r=-1.0), dict(tf=-1e-9), dict(tr=-1e-9),
              dict(max_dist=float("nan")), dict(method=-1), dict(method=3), dict(kernel=-1), dict(kernel=5),
              dict(k=0.0), dict(k=-0.03), dict(k=float("nan")))
    for method in range(3):
        own = (dict(eps=0.0), dict(eps=1.5), dict(eps=float("nan")), dict(eps=-1e-3)) if method == 2 else ()
        for bad in common + own:
            kw = dict(dict(method=method), **bad)
            assert _robust(L, **kw) == -1, kw
            assert _robust(L, **dict(kw, P=0)) == (0 if "P" in bad else -1), kw
        assert _robust(L, method=method, ptrs=0) == -1                 # NULL pairs / T0 / fitness / rmse / status
        assert _robust(L, method=method, T=0) == -1                    # NULL T
        assert _robust(L, method=method, index=0) == -1                # NULL index with M > 0
        assert _robust(L, method=method, index_bytes=L.mvr_radius_index_bytes(10) - 1) == -1   # a short index
    for method in (1, 2):
        assert _robust(L, method=method, normals=0) == -1              # NULL normals where the method reads them


# --------------------------------------------------------------------------------------------------- Python surface
def test_argument_errors():
    import torch
    from lib.icp import ROBUST_KERNELS, gicp_pair, gicp_refine, icp_pair, icp_refine
    assert ROBUST_KERNELS == RO.KERNELS
    T = np.tile(np.eye(4), (2, 1, 1))
    pairs = [[0, 1], [1, 0]]
    fo = types.SimpleNamespace(r=0.075, M=10, xyz=torch.zeros(10, 3, dtype=torch.float64),
                               normals=torch.zeros(10, 3, dtype=torch.float64))     # never touched: errors come first
    bad = (dict(kernel="l1"), dict(kernel="Tukey"), dict(kernel=4), dict(kernel="tukey"),
           dict(kernel="huber", kernel_k=0.0), dict(kernel="cauchy", kernel_k=-0.01),
           dict(kernel="gm", kernel_k=float("nan")), dict(kernel_k=0.03),
           dict(return_weight_sum=True))
    for kw in bad:
        for method in ("point_to_point", "point_to_plane"):
            with pytest.raises(ValueError, match="kernel"):
                icp_refine(fo, pairs, T, method=method, **kw)
        with pytest.raises(ValueError, match="kernel"):
            gicp_refine(fo, pairs, T, **kw)
        with pytest.raises(ValueError, match="kernel"):
            icp_pair(np.zeros((10, 3)), np.zeros((12, 3)), np.eye(4), **kw)
        with pytest.raises(ValueError, match="kernel"):
            gicp_pair(np.zeros((10, 3)), np.zeros((12, 3)), np.eye(4), **kw)
    with pytest.raises(ValueError, match="normals"):                    # a kernel does not lift the other checks
        icp_refine(types.SimpleNamespace(r=0.075), pairs, T, method="point_to_plane", kernel="tukey", kernel_k=0.03)
    with pytest.raises(ValueError):
        icp_refine(fo, pairs, T, max_dist=0.08, kernel="tukey", kernel_k=0.03)


def test_register_scene_argument_errors():
    from lib.multiview import register_scene
    clouds = [np.zeros((4, 3), np.float32)] * 2
    for kw in (dict(icp_kernel="l1"), dict(icp_kernel_k=0.03), dict(icp_kernel="tukey", icp_kernel_k=0.0),
               dict(icp_kernel="huber", icp_kernel_k=float("nan"))):
        with pytest.raises(ValueError, match="kernel"):                 # before any device work
            register_scene(clouds, **kw)


def test_command_line_parsing():
    from scripts.register_scene import check_args, parse_icp_kernel, parser
    assert parse_icp_kernel("tukey") == ("tukey", None) and parse_icp_kernel("gm:0.000625") == ("gm", 0.000625)
    assert parse_icp_kernel("l2") == ("l2", None) and parse_icp_kernel("huber:2e-2") == ("huber", 0.02)
    for bad in ("l1", "", "tukey:", "tukey:0", "tukey:-1", "tukey:nan", "tukey:x", "tukey:0.03:1", "Tukey", ":0.03"):
        with pytest.raises(ValueError, match="--icp_kernel"):
            parse_icp_kernel(bad)
    ap = parser()
    base = ["--fragments", "a.ply", "b.ply", "--out", "o"]
    assert check_args(ap, ap.parse_args(base)).icp_kernel is None
    assert check_args(ap, ap.parse_args(base + ["--icp_kernel", "cauchy:0.05"])).icp_kernel == ("cauchy", 0.05)
    with pytest.raises(SystemExit):
        check_args(ap, ap.parse_args(base + ["--icp_kernel", "l1"]))
