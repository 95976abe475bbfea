"""CPU-side facts the GPU comparison of tests/test_gpu_fgr.py rests on, pinned on the numpy restatement
(tests/fgr_oracle.py) of exactly the batch that test runs; lib.utils.run_fgr_batch's argument checks; mvr_fgr's scalar
checks and its empty call (no device needed: they return before any HIP call)."""
import inspect
import os

import numpy as np
import pytest

from conftest import PKG
import fgr_oracle as F

LIB = os.path.join(PKG, "libmvreg_hip.so")
FITTED = [p for p, (n, _) in enumerate(F.CASES) if n >= 3]


def test_tuple_comparisons_are_far_from_equality():
    """the set of passing tuple tests is compared exactly: no comparison between distinct draws may be within 1e-9
    relative of equality (measured: the smallest gap is 2.8e-7, at case 11)"""
    gaps = [r["gap"] for r in F.batch_results(True)]
    print("smallest relative gaps per case: %s" % ["%.2e" % g for g in gaps])
    assert all(g == np.inf for g in gaps[:3])
    assert min(gaps) > 1e-9
    assert int(np.argmin(gaps)) == 11 and 2e-7 < gaps[11] < 4e-7


def test_tuple_counts_exercise_both_sides_of_the_cap():
    res = F.batch_results(True)
    assert [res[p]["n_tuples"] for p in (5, 10)] == [1000, 1000]
    assert [res[p]["full_at"] for p in (5, 10)] == [2032, 8204]
    assert [res[p]["n_tuples"] for p in (6, 7, 8, 9)] == [813, 740, 702, 842]
    assert all(res[p]["full_at"] == -1 for p in (3, 4, 6, 7, 8, 9, 11))
    assert res[11]["n_tuples"] == 115 and F.CASES[11][0] * F.DEFAULTS["tuple_factor"] == 200000
    for r in res:
        assert r["n_used"] == 3 * r["n_tuples"]
    for p, r in enumerate(F.batch_results(False)):
        assert r["n_tuples"] == 0 and r["n_used"] == (F.CASES[p][0] if p in FITTED else 0)
    # both sides of a chunk of one test per thread at 256, 512 and 1024 threads: caps reached in a later chunk
    # (2032, 8204), lists that end below a chunk (300 tests at n = 3) and beyond many (200000 tests)
    assert res[3]["n_tuples"] > 0 and 3 * F.DEFAULTS["tuple_factor"] < 1024 < 2032


def test_no_final_distance_at_the_threshold():
    """fitness is an inlier count: no row may end within 1e-7 relative of max_dist"""
    for tt in (True, False):
        for p in FITTED:
            d = F.batch_results(tt)[p]["dist"]
            assert np.abs(d - F.MAX_DIST).min() > 1e-7 * F.MAX_DIST, (tt, p)


def test_status_and_identity_of_the_short_cases():
    for tt in (True, False):
        res = F.batch_results(tt)
        for p in range(3):
            assert res[p]["status"] == 1 and np.array_equal(res[p]["T"], np.eye(4))
            assert res[p]["fitness"] == 0.0 and res[p]["rmse"] == 0.0 and (res[p]["trace"] == -1.0).all()
        assert all(res[p]["status"] == 0 for p in FITTED)


def test_recovery_against_the_truth():
    """with the tuple filter every case with n >= 3 ends within 1 degree and 0.02 m (measured: at most 0.38 degrees
    and 0.007 m, cases 3 and 4, the 5 mm noise on 3 to 4 points); without it cases 3-10 do, and case 11 (5 % inliers)
    does not (119 degrees off): what the filter is for"""
    for tt, cases in ((True, FITTED), (False, range(3, 11))):
        for p in cases:
            _, _, R, t = F.case(p)
            deg, m = F.pose_error(F.batch_results(tt)[p]["T"], R, t)
            print("tuple filter %s case %d: %.3f deg, %.4f m" % (tt, p, deg, m))
            assert deg < 1.0 and m < 0.02, (tt, p, deg, m)
    _, _, R, t = F.case(11)
    deg, m = F.pose_error(F.batch_results(False)[11]["T"], R, t)
    print("no filter, case 11: %.1f deg, %.3f m" % (deg, m))
    assert deg > 10.0


def test_trace_follows_the_schedule():
    """mu is divided by 1.4 at k = 0, 4, 8, .. while it is above delta^2, and never clamped"""
    r = F.batch_results(True)[10]
    mu = r["trace"][:, 0]
    assert mu[0] == 1.0 / 1.4 and (mu[:-1] >= mu[1:]).all() and (mu.reshape(-1, 4) == mu[::4, None]).all()
    assert np.isclose(mu[-1], 1.4 ** -16, rtol=1e-13, atol=0)   # delta^2 = (0.05 / scale)^2 is never reached
    assert (r["trace"][:, 1] >= 0.0).all()


def test_sensitivity_to_the_last_bits():
    """inputs perturbed by 1e-15 relative move T by less than 1e-12 (measured: at most 1.3e-15, the cases that do not
    converge included): the GPU's 1e-9 bound leaves orders of margin over a reordered sum"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for tt in (True, False):
        for p in FITTED:
            x1, x2, _, _ = F.case(p)
            y1 = x1 * (1.0 + 1e-15 * rng.uniform(-1, 1, x1.shape))
            y2 = x2 * (1.0 + 1e-15 * rng.uniform(-1, 1, x2.shape))
            got = F.fgr(y1, y2, seed=F.SEED, p=p, tuple_test=tt)
            want = F.batch_results(tt)[p]
            assert got["n_tuples"] == want["n_tuples"]
            worst = max(worst, float(np.abs(got["T"] - want["T"]).max()))
    print("largest |dT| under a 1e-15 relative perturbation: %.2e" % worst)
    assert worst < 1e-12


def test_degenerate_and_invalid_inputs():
    line = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]])
    r = F.fgr(line, line + [0.5, 0.25, -1.0], tuple_test=False)
    assert r["status"] == 8 and np.array_equal(r["T"][:3, :3], np.eye(3))
    np.testing.assert_allclose(r["T"][:3, 3], [0.5, 0.25, -1.0], atol=1e-15)
    assert r["trace"][0, 0] == 1.0 / 1.4 and (r["trace"][1:] == -1.0).all()
    bad = line.copy()
    bad[1, 2] = np.nan
    assert F.fgr(bad, line, tuple_test=False)["status"] == 4
    same = np.ones((5, 3))
    assert F.fgr(same, same * 2.0, tuple_test=False)["status"] == 1


# ------------------------------------------------------------------------------------------- the Python surface
def test_run_fgr_batch_signature_and_argument_checks():
    from lib.utils import RANSAC_DIST, run_fgr_batch
    sig = inspect.signature(run_fgr_batch)
    want = dict(counts=None, seed=0, max_dist=RANSAC_DIST, iters=64, division_factor=1.4, tuple_test=True,
                tuple_scale=0.95, max_tuples=1000, tuple_factor=100, device=None, return_trace=False)
    assert list(sig.parameters) == ["xyz_i", "xyz_j"] + list(want)
    assert {k: sig.parameters[k].default for k in want} == want
    x = np.zeros((2, 5, 3))
    for bad in (dict(max_dist=0.0), dict(max_dist=float("inf")), dict(max_dist=float("nan")), dict(iters=-1),
                dict(division_factor=1.0), dict(division_factor=float("inf")), dict(max_tuples=0),
                dict(tuple_factor=0), dict(tuple_factor=-1), dict(tuple_scale=0.0), dict(tuple_scale=1.5),
                dict(tuple_factor=1 << 30), dict(counts=[1, 2, 3]), dict(counts=[6, 0]), dict(counts=[-1, 0])):
        with pytest.raises(ValueError):
            run_fgr_batch(x, x, **bad)
    for a, b in ((np.zeros((5, 3)), np.zeros((5, 3))), (x, np.zeros((2, 4, 3))), (np.zeros((2, 5, 2)),) * 2):
        with pytest.raises(ValueError):
            run_fgr_batch(a, b)


def test_register_scene_and_cli_argument_checks():
    from lib import multiview as MV
    assert inspect.signature(MV.register_scene).parameters["coarse"].default == "ransac"
    with pytest.raises(ValueError, match="coarse"):
        MV.register_scene([None, None], 0.025, coarse="teaser")
    with pytest.raises(ValueError, match="ransac_checkers"):
        MV.register_scene([None, None], 0.025, coarse="fgr", ransac_checkers=True)
    from scripts import register_scene as S
    ap = S.parser()
    assert ap.parse_args(["--fragments", "a", "b", "--out", "o"]).coarse == "ransac"
    assert S.check_args(ap, ap.parse_args(["--fragments", "a", "b", "--out", "o", "--coarse", "fgr"])).coarse == "fgr"
    with pytest.raises(SystemExit):
        S.check_args(ap, ap.parse_args(["--fragments", "a", "b", "--out", "o", "--coarse", "fgr", "--checkers"]))
    with pytest.raises(SystemExit):
        ap.parse_args(["--fragments", "a", "b", "--out", "o", "--coarse", "teaser"])
    from scripts import pairwise_demo as D
    dp = D.parser()
    assert D.check_args(dp.parse_args(["cfg", "--fpfh", "--fgr"])).fgr
    with pytest.raises(ValueError, match="--fpfh"):
        D.check_args(dp.parse_args(["cfg", "--fgr"]))
    with pytest.raises(ValueError, match="--checkers"):
        D.check_args(dp.parse_args(["cfg", "--fpfh", "--fgr", "--checkers"]))


# ------------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")
def test_mvr_fgr_scalar_checks_come_before_the_empty_call():
    from lib import _native
    L = _native.lib()
    Z = None

    def call(P=0, stride=0, max_dist=0.05, iters=64, div=1.4, tf=100, mt=1000, ts=0.95, ws=0):
        return L.mvr_fgr(Z, Z, stride, Z, P, max_dist, iters, div, tf, mt, ts, 0, Z, Z, Z, Z, Z, Z, Z, Z, ws, Z)
    assert call() == 0 and call(tf=0, ts=7.0) == 0 and call(iters=0) == 0
    for bad in (dict(P=-1), dict(P=1 << 23), dict(iters=-1), dict(max_dist=0.0), dict(max_dist=float("inf")),
                dict(max_dist=float("nan")), dict(div=1.0), dict(div=float("nan")), dict(div=float("inf")),
                dict(tf=-1), dict(ts=0.0), dict(ts=1.0001), dict(ts=float("nan")), dict(mt=0),
                dict(stride=3 * (1 << 25), tf=100)):
        assert call(**bad) == -1, bad
    assert call(ts=1.0) == 0
    # with pairs: NULL pointers and a short workspace are refused
    assert L.mvr_fgr_workspace_bytes(2, 2000, 1000) == 2 * 3000 * 48
    assert L.mvr_fgr_workspace_bytes(2, 5000, 1000) == 2 * 5000 * 48 and L.mvr_fgr_workspace_bytes(0, 5, 5) == 0
    assert call(P=1, stride=15, ws=1 << 20) == -1
    assert call(P=1, stride=6000, ws=8) == -1
