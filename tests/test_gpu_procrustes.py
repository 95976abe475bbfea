"""mvr_procrustes / mvr_procrustes_f64 (csrc/procrustes.hip) and the 3 x 3 Jacobi SVD behind them
(csrc/svd3.hpp) against tests/procrustes_oracle.py (two-pass long-double Kabsch, fp64 LAPACK SVD), through the C
ABI: the reflection and rank-deficient branches of the SVD, the tail of the workgroup reduction, both point
layouts, inputs far from the origin, status = 1 and power-of-two weight scales.  tests/test_procrustes_host.py
shows that every compared case has a gap g = (s1 + d s2) / s0 >= 0.05: nothing is skipped here.

Tolerances (EPS64 = 2^-53, EPS32 = 2^-24, unit roundoffs; none is fitted to the kernel):
  R, fp64      1e-12: a rotation from a 3 x 3 SVD moves by <= (perturbation of H / s0) / g; the fp64 solve
               perturbs H by ~EPS64 per operation: 1.1e-16 * (1/g <= 20) * ~100 operations = 2.2e-13.
  R, fp32      5e-7 fed, 1e-6 on point clouds: the solve is fp64 on the fp32-rounded inputs, so the error is
               the rounding of R's entries to fp32, <= EPS32 = 6e-8; the bounds leave a factor of 8 and 16.
  R, far       1e-11 in fp64: 50 x the 2e-13 that test_procrustes_host.py holds plain two-pass fp64 numpy to
               (it measures 1.4e-15 on these clouds).
  rotation     |R^T R - I|, |det R - 1| <= 1e-13 (fp64: V and U are products of <= 90 Givens rotations, each
               orthogonal to EPS64), 5e-7 (fp32: nine entries rounded by <= EPS32, three products per sum).
  tr(R H)      >= optimum - 1e-12 s0 in fp64.  In fp32 R is rounded entry by entry, which is first order in
               tr(R H): <= 9 * EPS32 * s0 = 5.4e-7 s0 -> 5e-7 s0 is asked.  (One point, N = 1, has H = W (eps /
               (W + eps))^2 x1 x2^T, ~1e-14 of the raw moments: moments about the origin missed the optimum there
               by 1.7e-5 s0 (fp64) and 9.4e-5 s0 (fp32) on an MI355X; about the pair's first point: 3e-16, 2e-8.)
  t            |t - (mu2 - R_gpu mu1)| <= 64 EPS64 (1 + |mu1| + |mu2|) (fp64), 8 EPS32 (...) (fp32).
  res          against ||R_gpu x1 + t_gpu - x2|| in fp64: 1e-12 (fp64), 4 EPS32 (1 + max |x|) (fp32).
"""
import functools

import numpy as np
import pytest

import procrustes_oracle as O

pytestmark = pytest.mark.gpu

EPS64, EPS32 = 2.0 ** -53, 2.0 ** -24
DTYPES = (np.float64, np.float32)
SENT = -777.25          # exactly representable in fp32: the sentinel of every float output
ISENT = -77


def _is64(dt):
    return np.dtype(dt) == np.float64


def run(gpu, x1, x2, w, normalize, eps, dt, interleaved=False, want_res=True):
    """One launch on [P,N,3] points.  Separate arrays (x_nstride 3, w and res rows of N) or, interleaved, one
    [P,N,6] array (x2 = x1 + 3, x_nstride 6) with w and res rows of N + 5.  Every output sits inside a larger
    buffer of sentinels, which must come back untouched; so must w (no guard is asked for)."""
    import torch
    from lib import _native as NV
    tdt = torch.float64 if _is64(dt) else torch.float32
    P, N, _ = x1.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)   # noqa: E731
    x1, x2 = np.asarray(x1).astype(dt), np.asarray(x2).astype(dt)
    if interleaved:
        xs = dev(np.concatenate([x1, x2], axis=2))
        p1, p2, xps, xns = xs.data_ptr(), xs.data_ptr() + 3 * xs.element_size(), N * 6, 6
        ld = N + 5
    else:
        a, b = dev(x1), dev(x2)
        p1, p2, xps, xns, ld = a.data_ptr(), b.data_ptr(), N * 3, 3, N
    wbuf = None
    if w is not None:
        wnp = np.full((P, ld), SENT, dt)
        wnp[:, :N] = np.asarray(w).astype(dt)
        wbuf = dev(wnp)
    R = torch.full((P + 2, 9), SENT, dtype=tdt, device=gpu)
    t = torch.full((P + 2, 3), SENT, dtype=tdt, device=gpu)
    res = torch.full((P + 2, ld), SENT, dtype=tdt, device=gpu)
    status = torch.full((P + 2,), ISENT, dtype=torch.int32, device=gpu)
    L = NV.lib()
    fn = L.mvr_procrustes_f64 if _is64(dt) else L.mvr_procrustes
    rc = fn(NV.c_vp(p1), NV.c_vp(p2), xps, xns, NV.ptr(wbuf), ld, None, None, 0, P, N, int(normalize), eps,
            NV.ptr(R[1]), NV.ptr(t[1]), NV.ptr(res[1]) if want_res else None, ld, None, 0, NV.ptr(status[1:]), 0,
            NV.stream())
    assert rc == 0
    torch.cuda.synchronize()
    R, t, res, status = R.cpu().numpy(), t.cpu().numpy(), res.cpu().numpy(), status.cpu().numpy()
    for o in (R, t, res):
        assert np.all(o[0] == SENT) and np.all(o[-1] == SENT)
    assert np.all(res[:, N:] == SENT) and status[0] == ISENT and status[-1] == ISENT
    if not want_res:
        assert np.all(res == SENT)
    if w is not None:
        assert np.array_equal(wbuf.cpu().numpy(), wnp, equal_nan=True)
    return R[1:-1].reshape(P, 3, 3), t[1:-1], res[1:-1, :N], status[1:-1]


def check_rotation(R, dt, what):
    tol = 1e-13 if _is64(dt) else 5e-7
    orth, det = O.rotation_defects(R)
    assert np.all(np.isfinite(R)), what
    assert orth <= tol and det <= tol, (what, orth, det)


def check_optimal(R, ref, p, dt, what):
    """tr(R H) reaches the optimum (the module docstring has the bounds)"""
    s0 = ref["s"][p, 0]
    slack = (1e-12 if _is64(dt) else 5e-7) * s0
    gain = O.trace_gain(R, ref["H"][p])
    print("%s pair %d: optimum - tr(R H) = %.3g s0" % (what, p, (ref["opt"][p] - gain) / s0 if s0 > 0 else 0.0))
    assert gain >= ref["opt"][p] - slack, (what, gain, ref["opt"][p], s0)


def check_t(R, t, ref, dt, what):
    """t against mu2 - R_gpu mu1 with the oracle's means"""
    for p in range(len(R)):
        lim = (64 * EPS64 if _is64(dt) else 8 * EPS32) * (1 + np.linalg.norm(ref["mu1"][p])
                                                            + np.linalg.norm(ref["mu2"][p]))
        err = np.abs(t[p].astype(np.float64) - (ref["mu2"][p] - R[p].astype(np.float64) @ ref["mu1"][p])).max()
        assert err <= lim, (what, p, err, lim)


def check_res(R, t, res, x1, x2, dt, what):
    """the second pass alone: res against ||R_gpu x1 + t_gpu - x2|| recomputed in fp64"""
    x1, x2 = np.asarray(x1).astype(dt).astype(np.float64), np.asarray(x2).astype(dt).astype(np.float64)
    R, t, res = R.astype(np.float64), t.astype(np.float64), res.astype(np.float64)
    for p in range(len(R)):
        own = np.linalg.norm(x1[p] @ R[p].T + t[p] - x2[p], axis=1)
        lim = 1e-12 if _is64(dt) else 4 * EPS32 * (1 + max(np.abs(x1[p]).max(), np.abs(x2[p]).max()))
        assert np.abs(res[p] - own).max() <= lim, (what, p, np.abs(res[p] - own).max(), lim)


@functools.lru_cache(maxsize=None)
def _fed_ref(which, dt):
    H = (O.svd_unique_cases if which == "A" else O.svd_nonunique_cases)()[0]
    return O.solve_fed(H, dt)


# ------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("dt", DTYPES)
def test_svd_unique_solves(gpu, dt):
    """A: 93 matrices through feed(H) in one launch — Gaussian (32 with det < 0: d = -1), diagonal in every
    order and sign (the ga == 0 skip, the column sort, reflection without rotation), rotations (R = H^T), exactly
    rank-2 ones (zero columns and rows included: the cross-product completion)."""
    H, kinds = O.svd_unique_cases()
    x1, x2 = O.feed(H)
    ref = _fed_ref("A", dt)
    R, t, res, status = run(gpu, x1, x2, None, 0, 0.0, dt)
    assert np.all(status == 0)
    err = np.abs(R - ref["R"]).reshape(len(H), -1).max(1)
    for kind in sorted(set(kinds)):
        print("A %s %-8s max |R - R_oracle| %.3g" % (np.dtype(dt).name, kind, err[np.array(kinds) == kind].max()))
    tol = 1e-12 if _is64(dt) else 5e-7
    assert err.max() <= tol, [(kinds[i], err[i]) for i in np.argsort(-err)[:5]]
    rot = np.array(kinds) == "rot"
    assert np.abs(R[rot] - np.swapaxes(H[rot], 1, 2)).max() <= tol
    # on the dyadic grid every partial sum of x2 is exact: t is exactly zero.  A rotation's entries are not on
    # it: t is a sum of six terms <= 1/2 that cancel, over 6 — a dozen roundings of values <= 3, over 6, and one
    # more of a value <= 1/2
    assert np.all(t[~rot] == 0.0)
    assert np.abs(t[rot]).max() <= 8 * EPS64
    for p in range(len(H)):
        check_rotation(R[p], dt, kinds[p])
    check_res(R, t, res, x1, x2, dt, "A")


# ------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("dt", DTYPES)
def test_svd_nonunique_solves_properties(gpu, dt):
    """B: rank 1, zero, -I, diag(2,1,-1), Q diag(2,1,1) P with det < 0 — the rotation is not unique: it must be
    a rotation and reach the optimum of tr(R H), which is."""
    H, kinds = O.svd_nonunique_cases()
    x1, x2 = O.feed(H)
    ref = _fed_ref("B", dt)
    R, t, res, status = run(gpu, x1, x2, None, 0, 0.0, dt)
    assert np.all(status == 0)
    for p in range(len(H)):
        check_rotation(R[p], dt, kinds[p])
        check_optimal(R[p], ref, p, dt, kinds[p])
    z = kinds.index("zero")
    assert np.array_equal(R[z], np.eye(3)) and np.all(t[z] == 0.0)


# ------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", O.REDUCTION_N)
def test_reduction_shapes(gpu, N, dt, interleaved):
    """C: N below, at and over one pass of the 256-thread workgroup, a quarter of the weights exactly zero, in
    separate arrays and in the OANet layout with padded w / res rows"""
    x1, x2, w = O.reduction_case(N)
    ref = O.kabsch_ld(x1, x2, w, True, 1e-7, dt)
    R, t, res, status = run(gpu, x1, x2, w, 1, 1e-7, dt, interleaved)
    assert np.all(status == 0)
    what = "C N=%d %s %s" % (N, np.dtype(dt).name, "interleaved" if interleaved else "separate")
    if N >= 3:
        err = np.abs(R - ref["R"]).max()
        print("%s: max |R - R_oracle| %.3g" % (what, err))
        assert err <= (1e-12 if _is64(dt) else 1e-6), what
    else:
        for p in range(3):
            check_rotation(R[p], dt, what)
            check_optimal(R[p], ref, p, dt, what)
    if N >= 3:
        check_t(R, t, ref, dt, what)
    check_res(R, t, res, x1, x2, dt, what)


def test_no_residuals_asked(gpu):
    """res = NULL: nothing is written past R, t, status"""
    x1, x2, w = O.reduction_case(257)
    for dt in DTYPES:
        R, t, _, _ = run(gpu, x1, x2, w, 1, 1e-7, dt, want_res=False)
        R2, t2, _, _ = run(gpu, x1, x2, w, 1, 1e-7, dt)
        assert np.array_equal(R, R2) and np.array_equal(t, t2)


# ------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("dt,c", [(dt.type, c) for dt, cs in O.FAR_C.items() for c in cs])
def test_far_from_the_origin(gpu, dt, c):
    """D: a cloud of spread 1 at distance c.  The covariance must not be formed from raw moments of size c^2.
    Worst |R - R_oracle| over the four pairs, fp64, measured on an MI355X:
        c        raw moments about the origin    moments about the pair's first point
        1e2      1.0e-12                         3.3e-15
        1e3      3.1e-11                         8.9e-16
        1e4      4.7e-9                          6.1e-16
    (fp32 entry point, either origin: 2.7e-8 at 1e2, 3.0e-8 at 1e3 — the rounding of R.)"""
    x1, x2, w = O.far_case(c)
    ref = O.kabsch_ld(x1, x2, w, True, 1e-7, dt)
    R, t, res, status = run(gpu, x1, x2, w, 1, 1e-7, dt)
    assert np.all(status == 0)
    err = np.abs(R - ref["R"]).max()
    print("D %s c=%g: max |R - R_oracle| %.3g" % (np.dtype(dt).name, c, err))
    assert err <= (1e-11 if _is64(dt) else 1e-6)
    if _is64(dt):
        check_t(R, t, ref, dt, "D c=%g" % c)


# ------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("dt", DTYPES)
def test_status_flags_a_non_finite_pair_only(gpu, dt):
    """E: one NaN in x2, or +inf in w, of pair 1 -> status [0,1,0], R = I and t = 0 there, the other pairs
    bit-equal to the clean call; kabsch_transformation_estimation reports it as its flag."""
    import torch
    from lib.utils import kabsch_transformation_estimation
    x1, x2, w = O.plain_case(100)
    clean = run(gpu, x1, x2, w, 1, 1e-7, dt)
    assert np.all(clean[3] == 0)
    tt = lambda a: torch.from_numpy(a.astype(dt)).to(gpu)   # noqa: E731
    bad_x2, bad_w = x2.copy(), w.copy()
    bad_x2[1, 5, 1] = np.nan
    bad_w[1, 7] = np.inf
    for what, (b2, bw) in (("NaN in x2", (bad_x2, w)), ("+inf in w", (x2, bad_w))):
        R, t, res, status = run(gpu, x1, b2, bw, 1, 1e-7, dt)
        assert list(status) == [0, 1, 0], what
        assert np.array_equal(R[1], np.eye(3)) and np.all(t[1] == 0.0), what
        for p in (0, 2):
            assert np.array_equal(R[p], clean[0][p]) and np.array_equal(t[p], clean[1][p]), what
            assert np.array_equal(res[p], clean[2][p]), what
        Rk, tk, _, flag = kabsch_transformation_estimation(tt(x1), tt(b2), tt(bw))
        assert flag is True, what
        assert np.array_equal(Rk.cpu().numpy(), R) and np.array_equal(tk.cpu().numpy()[:, :, 0], t), what
    assert kabsch_transformation_estimation(tt(x1), tt(x2), tt(w))[3] is False


# ------------------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("dt", DTYPES)
def test_weight_scale_by_powers_of_two_is_exact(gpu, dt):
    """F: normalize = 0, eps = 0: every moment scales by an exact power of two and every threshold of the
    Jacobi SVD is relative, so w, w 2^-60 and w 2^60 give the same bits"""
    x1, x2, w = O.plain_case(300)
    base = run(gpu, x1, x2, w, 0, 0.0, dt)
    ref = O.kabsch_ld(x1, x2, w, False, 0.0, dt)
    assert np.abs(base[0] - ref["R"]).max() <= (1e-12 if _is64(dt) else 1e-6)
    for k in (-60, 60):
        R, t, res, status = run(gpu, x1, x2, w * 2.0 ** k, 0, 0.0, dt)
        assert np.all(status == 0)
        assert np.array_equal(R, base[0]) and np.array_equal(t, base[1]) and np.array_equal(res, base[2]), k
