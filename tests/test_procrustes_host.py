"""CPU-side checks of the Procrustes reference (tests/procrustes_oracle.py) and of the conditions the GPU
comparisons of tests/test_gpu_procrustes.py rest on: every compared case is well conditioned (g >= 0.05, so no
case is skipped on the GPU), the cases meant to reflect do, feed(H) delivers H exactly, and plain two-pass fp64
stays within 2e-13 of the long-double reference far from the origin (what the GPU's 1e-11 there is set over; on
these clouds it measures 1.4e-15)."""
import numpy as np
import pytest

import procrustes_oracle as O
from oracle.kabsch import kabsch


def _props(R, H, opt, s0, tol, tol_tr):
    orth, det = O.rotation_defects(R)
    assert np.all(np.isfinite(R)) and orth <= tol and det <= tol, (orth, det)
    assert O.trace_gain(R, H) >= opt - tol_tr * s0, (O.trace_gain(R, H), opt)


def test_kabsch_ld_matches_the_fp64_restatement_near_the_origin():
    x1, x2, w = O.plain_case()
    for wts, norm, eps in ((w, True, 1e-7), (None, True, 1e-7), (w, False, 0.0)):
        r = O.kabsch_ld(x1, x2, wts, norm, eps)
        Ro, to, _, flag = kabsch(x1, x2, wts, norm, eps)
        assert not flag
        np.testing.assert_allclose(r["R"], Ro, rtol=0, atol=1e-12)
        np.testing.assert_allclose(r["t"], to[:, :, 0], rtol=0, atol=1e-12)
        assert r["g"].min() > 1.0 and np.all(r["d"] == 1.0)


def test_feed_reproduces_H_exactly():
    for H in (O.svd_unique_cases()[0], O.svd_nonunique_cases()[0]):
        x1, x2 = O.feed(H)
        for dt in (np.float64, np.float32):
            a, b = x1.astype(dt).astype(np.float64), x2.astype(dt).astype(np.float64)
            cov = np.einsum("pni,pnj->pij", a, b)
            exact = np.array([O.on_grid(h) for h in H])
            if dt == np.float64:
                assert np.array_equal(cov, H)
            assert np.array_equal(cov[exact], H[exact])
            assert np.array_equal(O.solve_fed(H, dt)["H"][exact], H[exact])
            # both means are exactly zero, in whatever order the six terms are added: on the grid every partial
            # sum is exact
            for perm in (np.arange(6), np.array([0, 4, 2, 1, 5, 3]), np.array([5, 1, 3, 0, 2, 4])):
                for x in (a, b[exact]):
                    s = np.zeros((x.shape[0], 3))
                    for n in perm:
                        s = s + x[:, n]
                    assert np.all(s == 0.0)


def test_unique_cases_are_well_conditioned_and_reflect_where_meant():
    H, kinds = O.svd_unique_cases()
    kinds = np.array(kinds)
    assert len(H) == 93
    for kind, n in (("gauss+", 32), ("gauss-", 32), ("diag", 5), ("rot", 8), ("rank2", 8), ("zerocol", 4),
                    ("zerorow", 4)):
        assert (kinds == kind).sum() == n
    on = np.array([O.on_grid(h) for h in H])
    assert np.all(on == (kinds != "rot"))
    for dt in (np.float64, np.float32):
        r = O.solve_fed(H, dt)
        print("%s: min g %.3f, d = -1 in %d of %d" % (np.dtype(dt).name, r["g"].min(), (r["d"] < 0).sum(), len(H)))
        assert r["g"].min() >= O.G_FLOOR
        assert np.all(r["d"][kinds == "gauss-"] == -1.0) and (kinds == "gauss-").sum() >= 24
        assert np.all(r["d"][kinds == "gauss+"] == 1.0)
        assert np.all(np.linalg.det(H[kinds == "gauss-"]) < 0)
        dg = r["d"][kinds == "diag"]
        assert list(dg) == [1.0, 1.0, 1.0, -1.0, -1.0]
        # exactly rank 2 (products of grid vectors): the third singular value is rounding only
        for kind in ("rank2", "zerocol", "zerorow"):
            assert np.all(r["s"][kinds == kind][:, 2] <= 1e-13 * r["s"][kinds == kind][:, 0])
        # for a rotation H = U V^T, so R = V U^T = H^T
        np.testing.assert_allclose(r["R"][kinds == "rot"], np.swapaxes(H[kinds == "rot"], 1, 2), rtol=0,
                                   atol=1e-14 if dt == np.float64 else 2e-7)
        assert np.all(r["t"] == 0.0)
        for p in range(len(H)):
            _props(r["R"][p], r["H"][p], r["opt"][p], r["s"][p, 0], 1e-13, 1e-12)


def test_nonunique_cases_are_not_unique_and_the_oracle_passes_their_checks():
    H, kinds = O.svd_nonunique_cases()
    assert len(H) == 15 and kinds.count("rank1") == 8
    r = O.solve_fed(H)
    assert np.all(r["g"] <= 1e-14), r["g"]
    assert np.all(r["d"][[k in ("-I", "diag(2,1,-1)") or k.startswith("Q") for k in kinds]] == -1.0)
    assert np.all(r["s"][np.array(kinds) == "rank1", 1] <= 1e-14 * r["s"][np.array(kinds) == "rank1", 0])
    for p in range(len(H)):
        _props(r["R"][p], r["H"][p], r["opt"][p], r["s"][p, 0], 1e-13, 1e-12)
    assert np.array_equal(r["R"][kinds.index("zero")], np.eye(3))


@pytest.mark.parametrize("N", O.REDUCTION_N)
def test_reduction_cases(N):
    x1, x2, w = O.reduction_case(N)
    assert x1.shape == (3, N, 3) and np.all((w == 0).sum(1) == N // 4) and np.all((w[w > 0] > 0.1) & (w[w > 0] < 1))
    for dt in (np.float64, np.float32):
        r = O.kabsch_ld(x1, x2, w, True, 1e-7, dt)
        print("N %d %s: g %s" % (N, np.dtype(dt).name, r["g"]))
        if N >= 3:
            assert r["g"].min() >= O.G_FLOOR
        for p in range(3):
            _props(r["R"][p], r["H"][p], r["opt"][p], r["s"][p, 0], 1e-13, 1e-12)


def test_far_cases_and_what_two_pass_fp64_reaches():
    worst = 0.0
    for dt, cs in O.FAR_C.items():
        for c in cs:
            x1, x2, w = O.far_case(c)
            assert x1.shape == (4, 257, 3)
            r = O.kabsch_ld(x1, x2, w, True, 1e-7, dt)
            assert r["g"].min() >= O.G_FLOOR
            d0 = np.linalg.norm(r["mu1"], axis=1)
            assert np.all(np.abs(d0 / c - 1) < 0.01)
            if dt == np.float64:
                Ro = kabsch(x1, x2, w, True, 1e-7)[0]
                dR = np.abs(Ro - r["R"]).max()
                print("c %g: two-pass fp64 numpy |R - R_ld| %.3g" % (c, dR))
                worst = max(worst, dR)
    assert worst <= 2e-13
