"""CPU checks of the checked RANSAC (csrc/ransac.hip mvr_ransac_checked): the numpy restatement
(tests/ransac_checked_oracle.py) against oracle/ransac.py and against hand-worked cases, the share of undecided
iterations on every input tests/test_gpu_ransac_checked.py runs, the quality case the feature exists for, and the
parts of the ABI and of the Python wrappers that return before any GPU call."""
import ctypes
import os

import numpy as np
import pytest

from conftest import PKG
from oracle import ransac as O
import ransac_checked_oracle as C

LIB = os.path.join(PKG, "libmvreg_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")


def test_vectorised_draws_and_fits_are_the_oracles():
    idx = C.draws_all(11, 2, 100, 4, 37)
    for it in (0, 1, 57, 99):
        assert idx[it].tolist() == O.draws(11, 2, it, 4, 37)
    assert C.draws_all((1 << 64) - 3, 5, 8, 8, 1000)[7].tolist() == O.draws((1 << 64) - 3, 5, 7, 8, 1000)
    x1, x2, _, _ = C.corr(50, 0.5, seed=1)
    idx = C.draws_all(3, 0, 20, 3, 50)
    R, t = C.umeyama_all(x1[idx], x2[idx])
    for it in range(20):
        if len(set(idx[it])) < 3:
            continue
        Ro, to = O.umeyama(x1[idx[it]], x2[idx[it]])
        np.testing.assert_allclose(R[it], Ro, rtol=0, atol=1e-12)
        np.testing.assert_allclose(t[it], to, rtol=0, atol=1e-12)


@pytest.mark.parametrize("ransac_n", [3, 4])
def test_checkers_off_equals_plain_ransac(ransac_n):
    x1, x2, _, _ = C.corr(37, 0.3, seed=4)
    T, fit, rmse, best, own, cnt, err = O.ransac(x1, x2, seed=5, ransac_n=ransac_n, iters=100, p=1)
    r = C.ransac_checked(x1, x2, seed=5, ransac_n=ransac_n, iters=100, max_validation=100, edge_sim=0.0,
                         check_dist=0.0, p=1, valid=np.arange(100), hyps=own)
    assert r["bits"].all() and r["n_pass"] == r["n_valid"] == 100 and not r["undecided"].any()
    assert r["valid"].tolist() == list(range(100))
    full = [it for it in range(100) if len(set(O.draws(5, 1, it, ransac_n, 37))) >= 3]
    np.testing.assert_allclose(r["own"][full], own[full], rtol=0, atol=1e-9)
    assert r["best_iter"] == best and r["fitness"] == fit and r["rmse"] == rmse and np.array_equal(r["T"], T)
    assert np.array_equal(r["cnt"], cnt) and np.array_equal(r["err"], err)
    # a pair with fewer correspondences than the sample: nothing passes
    r = C.ransac_checked(x1[:ransac_n - 1], x2[:ransac_n - 1], ransac_n=ransac_n, iters=10, edge_sim=0.0)
    assert r["n_pass"] == 0 and r["best_iter"] == -1 and np.array_equal(r["T"], np.eye(4)) and r["fitness"] == 0.0


def test_edge_check_by_hand_and_repeated_draws():
    """one triple: source edges 1, 1, sqrt 2; target edges 1, 0.95, sqrt 1.9025 -> length ratios 1, 0.95, 0.9753.
    Every sample of three distinct rows is that triangle: it passes at 0.9 and fails at 0.96 (0.95 < 0.96); a sample
    that draws a row twice never passes."""
    x1 = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    x2 = np.array([[0.0, 0, 0], [1, 0, 0], [0, 0.95, 0]])
    distinct = np.array([len(set(O.draws(7, 0, it, 3, 3))) == 3 for it in range(200)])
    assert 20 < distinct.sum() < 100          # 6 of 27 ordered triples
    r = C.ransac_checked(x1, x2, seed=7, iters=200, edge_sim=0.9, check_dist=0.0, max_dist=0.1)
    assert np.array_equal(r["bits"], distinct) and r["n_pass"] == distinct.sum() and not r["undecided"].any()
    assert r["best_iter"] in np.flatnonzero(distinct) and r["fitness"] == 1.0
    r = C.ransac_checked(x1, x2, seed=7, iters=200, edge_sim=0.96, check_dist=0.0, max_dist=0.1)
    assert not r["bits"].any() and r["best_iter"] == -1
    # at the very threshold (0.95^2 against 0.95^2 x 1) the comparison is flagged, not decided
    r = C.ransac_checked(x1, x2, seed=7, iters=200, edge_sim=0.95, check_dist=0.0, max_dist=0.1)
    assert np.array_equal(r["undecided"], distinct)
    # edge checker off: repeated draws are allowed again
    r = C.ransac_checked(x1, x2, seed=7, iters=200, edge_sim=0.0, check_dist=0.0, max_dist=0.1)
    assert r["bits"].all()


def test_distance_and_normal_checks_by_hand():
    """a pure translation with row 3 moved 0.4 further: three distinct rows that hold row 3 are no rigid image of
    their sources within 0.01, so a sample passes the distance check iff it does not hold row 3"""
    rng = np.random.default_rng(0)
    x1 = rng.uniform(-1, 1, (6, 3))
    x2 = x1 + np.array([0.5, -0.25, 1.0])
    x2[3] += np.array([0.0, 0.4, 0.0])
    idx = C.draws_all(2, 0, 300, 3, 6)
    distinct = np.array([len(set(i)) == 3 for i in idx])
    clean = distinct & ~(idx == 3).any(1)
    r = C.ransac_checked(x1, x2, seed=2, iters=300, edge_sim=0.5, check_dist=0.01, max_dist=0.01)
    assert r["bits"][clean].all() and not r["bits"][~distinct].any() and not r["undecided"].any()
    assert np.array_equal(r["bits"], clean) and r["fitness"] == 5 / 6 and clean[r["best_iter"]]
    # normals: all (0, 0, 1) on both sides pass under the identity rotation; a flipped target normal in row 0
    # rejects every sample that holds row 0
    n1 = np.tile([0.0, 0, 1], (6, 1))
    n2 = n1.copy()
    n2[0] = [0, 0, -1]
    rn = C.ransac_checked(x1, x2, seed=2, iters=300, edge_sim=0.5, check_dist=0.01, max_dist=0.01, n1=n1, n2=n2,
                          normal_cos=np.cos(np.deg2rad(10.0)))
    assert np.array_equal(rn["bits"], r["bits"] & ~(idx == 0).any(1))


def test_cap_keeps_the_first_passing_iterations():
    x1, x2, _, _ = C.corr(300, 0.8, seed=12)
    full = C.ransac_checked(x1, x2, seed=C.SEED, iters=1000, max_validation=1000, edge_sim=0.9, check_dist=0.05)
    assert full["n_pass"] > 64
    for cap in (1, 64):
        r = C.ransac_checked(x1, x2, seed=C.SEED, iters=1000, max_validation=cap, edge_sim=0.9, check_dist=0.05)
        assert r["n_pass"] == full["n_pass"] and r["n_valid"] == cap
        assert r["valid"].tolist() == np.flatnonzero(full["bits"])[:cap].tolist()
        assert r["best_iter"] in r["valid"] and len(r["cnt"]) == cap
        b, fit, rmse = O.select(full["cnt"][:cap], full["err"][:cap], 300)
        assert r["best_iter"] == full["valid"][b] and r["fitness"] == fit and r["rmse"] == rmse


def test_undecided_share_on_the_gpu_tests_inputs():
    """the condition under which the GPU tests' comparisons mean something: at most 1e-3 of the iterations of any
    input they run are too close to call (random fp64 inputs: none is expected)"""
    worst = 0.0
    for n in C.PARITY_N:
        (x1, x2), counts = C.parity_inputs(n)
        for iters in C.PARITY_ITERS:
            for edge, dist in C.MODES.values():
                for p in range(3):
                    m = counts[p]
                    r = C.ransac_checked(x1[p, :m], x2[p, :m], seed=C.SEED, iters=iters, max_validation=C.PARITY_CAP,
                                         edge_sim=edge, check_dist=dist, p=p)
                    worst = max(worst, r["undecided"].mean())
    (x1, x2, n1, n2), counts = C.parity_inputs(300, normals=True)
    for p in range(3):
        m = counts[p]
        r = C.ransac_checked(x1[p, :m], x2[p, :m], seed=C.SEED, iters=4097, max_validation=C.PARITY_CAP, p=p,
                             n1=n1[p, :m], n2=n2[p, :m], normal_cos=np.cos(np.deg2rad(C.NORMAL_DEG)))
        worst = max(worst, r["undecided"].mean())
    q = C.QUALITY
    x1, x2, _, _ = C.corr(q["n"], q["inl"], q["data_seed"])
    r = C.ransac_checked(x1, x2, seed=q["seed"], iters=q["iters"], max_validation=q["max_validation"],
                         edge_sim=q["edge_sim"], check_dist=C.MAX_DIST)
    worst = max(worst, r["undecided"].mean())
    print("largest undecided share: %.3g" % worst)
    assert worst <= 1e-3


def test_quality_case_checkers_find_what_plain_ransac_misses():
    """2000 correspondences, 5 % inliers, on the library's counter stream: 3-point samples, 100000 draws, edge 0.9 and
    distance 0.05 reach at least 0.9 of the planted share; 4-point samples and 2500 draws stay below half of it"""
    q = C.QUALITY
    x1, x2, R, t = C.corr(q["n"], q["inl"], q["data_seed"])
    r = C.ransac_checked(x1, x2, seed=q["seed"], iters=q["iters"], max_validation=q["max_validation"],
                         edge_sim=q["edge_sim"], check_dist=C.MAX_DIST)
    plain = O.ransac(x1, x2, seed=q["seed"], ransac_n=4, iters=2500)
    print("checked: fitness %.4f, %d of %d samples passed; plain: fitness %.4f" % (r["fitness"], r["n_pass"],
                                                                                  q["iters"], plain[1]))
    assert r["fitness"] >= 0.9 * q["inl"] and r["n_pass"] < q["max_validation"]
    assert plain[1] < 0.5 * q["inl"]
    np.testing.assert_allclose(r["T"][:3, :3], R, atol=2e-2)
    np.testing.assert_allclose(r["T"][:3, 3], t, atol=3e-2)


# ------------------------------------------------------------------------------------------------------------ ABI
def _call(L, P=1, ransac_n=3, iters=1000, max_dist=0.05, maxv=100, edge=0.9, dist=0.05, ncos=-1.0, ptrs=True,
          ws_bytes=None, drop=None):
    """mvr_ransac_checked with host addresses standing in for the device pointers: every call here returns before a
    launch, so none is dereferenced"""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.c_void_p(ctypes.addressof(buf)) if ptrs else None
    need = L.mvr_ransac_checked_workspace_bytes(P, iters, maxv)
    req = {k: a for k in ("x1", "x2", "n", "T", "fit", "rmse", "best", "n_pass", "n_valid", "ws")}
    if drop:
        req[drop] = None
    return L.mvr_ransac_checked(req["x1"], req["x2"], 0, req["n"], P, ransac_n, iters, max_dist, 0, maxv, edge, dist,
                                None, None, ncos, req["T"], req["fit"], req["rmse"], req["best"], req["n_pass"],
                                req["n_valid"], None, None, None, req["ws"], need if ws_bytes is None else ws_bytes,
                                None)


@needs_lib
def test_abi_empty_batch_accepts_null_pointers():
    from lib import _native
    L = _native.lib()
    assert _call(L, P=0, ptrs=False, ws_bytes=0) == 0
    assert L.mvr_ransac_checked_workspace_bytes(0, 1000, 100) == 0
    per_pair = L.mvr_ransac_checked_workspace_bytes(1, 100000, 2500)
    assert 2500 * (12 * 8 + 8 + 4 + 4) + 100000 // 8 <= per_pair <= 2500 * 112 + 100000 // 8 + 2048
    # the bits are the only part that grows with the iterations
    assert L.mvr_ransac_checked_workspace_bytes(1, 200000, 2500) - per_pair <= 100000 // 8 + 512


@needs_lib
@pytest.mark.parametrize("kw", [
    dict(P=-1), dict(P=1 << 23), dict(ransac_n=2), dict(ransac_n=9), dict(iters=0), dict(iters=1 << 30),
    dict(maxv=0), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_dist=float("inf")), dict(edge=-0.1),
    dict(edge=1.0), dict(edge=float("nan")), dict(dist=-1.0), dict(dist=float("inf")), dict(dist=float("nan")),
    dict(ncos=1.5), dict(ncos=-1.5), dict(ncos=float("nan")), dict(ws_bytes=16), dict(drop="x1"), dict(drop="x2"),
    dict(drop="n"), dict(drop="T"), dict(drop="fit"), dict(drop="rmse"), dict(drop="best"), dict(drop="n_pass"),
    dict(drop="n_valid"), dict(drop="ws"),
], ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_abi_rejects(kw):
    from lib import _native
    L = _native.lib()
    assert _call(L, **kw) == -1, kw
    # scalars are validated before the empty short-cut
    if "drop" not in kw and "ws_bytes" not in kw and "P" not in kw:
        assert _call(L, **dict(kw, P=0, ptrs=False, ws_bytes=0)) == -1, kw


def test_wrapper_argument_errors():
    from lib.utils import run_ransac_checked_batch
    x = np.zeros((1, 10, 3))
    for kw in (dict(edge_sim=1.0), dict(edge_sim=-0.5), dict(check_dist=-1.0), dict(check_dist=float("nan")),
               dict(max_validation=0), dict(iters=0), dict(normal_deg=10.0), dict(normals_i=x, normals_j=x),
               dict(normals_i=x, normal_deg=10.0), dict(normals_i=x, normals_j=x, normal_deg=200.0)):
        with pytest.raises(ValueError):
            run_ransac_checked_batch(x, x, **kw)


def test_register_fpfh_rejects_unknown_checker_options():
    from lib.fpfh import register_fpfh

    class Fo:
        fpfh = object()
    for bad in ({"edge": 0.9}, 1, "yes"):
        with pytest.raises(ValueError):
            register_fpfh(Fo(), [[0, 1]], checkers=bad)


def test_clis_take_the_checkers_flag():
    from scripts import pairwise_demo, register_scene
    a = register_scene.parser().parse_args(["--fragments", "a.ply", "b.ply", "--out", "o"])
    assert a.checkers is False
    assert register_scene.parser().parse_args(["--fragments", "a.ply", "b.ply", "--out", "o", "--checkers"]).checkers
    assert pairwise_demo.parser().parse_args(["cfg.yaml", "--fpfh"]).checkers is False
    assert pairwise_demo.parser().parse_args(["cfg.yaml", "--fpfh", "--checkers"]).checkers is True
