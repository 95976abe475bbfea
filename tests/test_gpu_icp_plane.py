"""GPU normal estimation (csrc/normals.hip mvr_estimate_normals) and point-to-plane ICP (csrc/icp_plane.hip
mvr_icp_refine_plane, lib/icp.py method='point_to_plane') against the numpy / sklearn oracle
(tests/icp_plane_oracle.py): normals on the scene and on small and awkward shapes, fixed iteration counts with the
full trace, convergence, ground truth, the status bits, batch and translation invariance, the Python surface and the
benchmark harness's --icp_method.

Tolerance: 1e-9 on normals (up to sign, where the relative eigen-gap is at least 1e-4: an eigenvector moves by about
eps |C| / gap ~ 1e-11), on T, fitness, rmse and the trace (the project's fp64 bound); n_nbr, n_corr, iters and status
exactly.  The loop comparisons feed the oracle the GPU's own normals, so sign and eigen-solver rounding stay out of
them.  test_icp_plane_host.py checks that no case used here has a neighbour, a correspondence, a stopping test or a
pivot test within rounding of a tie."""
import functools
import os
import sys

import numpy as np
import pytest

import icp_oracle as O
import icp_plane_oracle as PO

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
if HELPERS not in sys.path:
    sys.path.insert(0, HELPERS)

pytestmark = pytest.mark.gpu
TOL = 1e-9
GAP = 1e-4
SENTINEL = -77.0


@functools.lru_cache(maxsize=None)
def _fo():
    """the scene's centroids on an index of cell 0.075, with normals over that radius"""
    from lib.overlap import FragmentOverlap
    fo = FragmentOverlap(O.scene4()[0], "FCGF", 0.025)
    fo.estimate_normals()
    return fo


def _split(fo, x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    return [x[fo.off[b]:fo.off[b + 1]] for b in range(fo.B)]


@functools.lru_cache(maxsize=None)
def _six_starts():
    return O.scene4_starts(O.SIX, O.scene4_centroids())


@functools.lru_cache(maxsize=None)
def _six(max_dist, max_iters, tol):
    """(GPU result with trace, oracle results on the GPU's points and normals) of the six pairs"""
    from lib.icp import icp_refine
    fo = _fo()
    got = icp_refine(fo, O.SIX, _six_starts(), max_dist, max_iters, tol, tol, return_trace=True,
                     method="point_to_plane")
    want = PO.icp_plane_batch(_split(fo, fo.xyz), _split(fo, fo.normals), O.SIX, _six_starts(), max_dist, max_iters,
                              tol, tol)
    return got, want


def _compare(got, want, trace=True):
    for k, w in enumerate(want):
        for name in ("n_corr", "iters", "status"):
            assert int(got[name][k]) == w[name], (k, name, int(got[name][k]), w[name])
        if w["status"] & 4:      # T0 (possibly not finite) copied bit for bit
            assert got["T"][k][:3].tobytes() == np.ascontiguousarray(w["T"]).tobytes(), k
        dT = 0.0 if w["status"] & 4 else np.abs(got["T"][k][:3] - w["T"]).max()
        df, dr = abs(got["fitness"][k] - w["fitness"]), abs(got["rmse"][k] - w["rmse"])
        dtr = np.abs(got["trace"][k] - w["trace"]).max() if trace else 0.0
        print("pair %d: |dT| %.3g, |d fitness| %.3g, |d rmse| %.3g, |d trace| %.3g, iters %d, status %d"
              % (k, dT, df, dr, dtr, w["iters"], w["status"]))
        assert dT <= TOL and df <= TOL and dr <= TOL and dtr <= TOL, k
        np.testing.assert_array_equal(got["T"][k][3], [0.0, 0.0, 0.0, 1.0])


# ------------------------------------------------------------------------------------------------------------ normals
def _raw_normals(fo, radius, viewpoints=None):
    """mvr_estimate_normals on sentinel-filled output buffers -> (normals [M,3], n_nbr [M]) numpy"""
    import torch
    from lib import _native as N
    nrm = torch.full((fo.M, 3), SENTINEL, dtype=torch.float64, device=fo.device)
    cnt = torch.full((fo.M,), int(SENTINEL), dtype=torch.int32, device=fo.device)
    vp = None if viewpoints is None else torch.as_tensor(np.asarray(viewpoints, np.float64)).to(fo.device)
    N.check(N.lib().mvr_estimate_normals(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.off_dev), fo.B,
                                         fo.M, fo.r, radius, N.ptr(vp), N.ptr(nrm), N.ptr(cnt), N.stream()),
            "mvr_estimate_normals")
    return nrm.cpu().numpy(), cnt.cpu().numpy()


def _compare_normals(what, frags, got_n, got_c, want, max_left_out):
    """n_nbr exactly; normals up to sign within TOL wherever the oracle's relative eigen-gap is at least GAP"""
    w_n = np.concatenate([w["normals"] for w in want])
    w_c = np.concatenate([w["n_nbr"] for w in want])
    gap = np.concatenate([w["gap"] for w in want])
    assert len(w_n) == len(got_n) == sum(len(f) for f in frags)
    np.testing.assert_array_equal(got_c, w_c)
    assert not np.any(got_n == SENTINEL)
    np.testing.assert_allclose(np.linalg.norm(got_n, axis=1), 1.0, rtol=0, atol=1e-14)
    keep = gap >= GAP
    diff = np.minimum(np.abs(got_n - w_n).max(1), np.abs(got_n + w_n).max(1))
    print("%s: %d points, %d left out below the eigen-gap %g, largest difference up to sign %.3g"
          % (what, len(w_n), int((~keep).sum()), GAP, diff[keep].max() if keep.any() else 0.0))
    assert (~keep).mean() <= max_left_out
    assert (diff[keep] <= TOL).all()
    few = w_c < 3
    np.testing.assert_array_equal(got_n[few], np.tile([0.0, 0.0, 1.0], (int(few.sum()), 1)))


@pytest.mark.parametrize("radius", [0.075, 0.05])
def test_scene_normals_match_oracle(gpu, radius):
    fo = _fo()
    assert fo.r == 3 * 0.025 and abs(fo.max_points - 2600) < 200       # an index of cell 0.075
    frags = _split(fo, fo.xyz)
    got_n, got_c = _raw_normals(fo, radius)
    want = PO.estimate_normals_batch(frags, radius)
    _compare_normals("scene, radius %g" % radius, frags, got_n, got_c, want, 0.05)
    assert (np.concatenate([w["gap"] for w in want]) >= GAP).all()              # the scene leaves out none
    # with viewpoints: towards them everywhere, and the oracle's sign wherever the test is not within rounding
    vps = np.asarray([f.mean(0) + [0.3, -0.2, 1.5] for f in frags])
    vn, vc = _raw_normals(fo, radius, vps)
    np.testing.assert_array_equal(vc, got_c)
    np.testing.assert_array_equal(np.abs(vn), np.abs(got_n))                    # only the sign differs
    xyz = np.concatenate(frags)
    to_vp = np.concatenate([np.tile(vps[b], (len(f), 1)) for b, f in enumerate(frags)]) - xyz
    dots = np.einsum("ij,ij->i", vn, to_vp)
    assert (dots >= 0).all()
    w_n = np.concatenate([w["normals"] for w in PO.estimate_normals_batch(frags, radius, vps)])
    clear = np.abs(dots) >= 1e-6 * np.linalg.norm(to_vp, axis=1)
    assert clear.mean() > 0.99 and (np.abs(vn - w_n).max(1)[clear] <= TOL).all()
    if radius == 0.075:      # FragmentOverlap.estimate_normals: the same call, stored on the object
        assert fo.normals.cpu().numpy().tobytes() == got_n.tobytes()
        assert fo.n_nbr.cpu().numpy().tobytes() == got_c.tobytes()


def test_normals_on_small_shapes_in_one_batch(gpu):
    from lib.overlap import FragmentOverlap
    frags = PO.small_normals_case()
    fo = FragmentOverlap(frags, "3DMatch", radius=PO.SMALL_R_INDEX)
    assert tuple(np.diff(fo.off)) == PO.SMALL_SIZES and fo.r == PO.SMALL_R_INDEX
    for radius in (0.06, PO.SMALL_R_INDEX):                                     # radius < r_index, radius == r_index
        got_n, got_c = _raw_normals(fo, radius)
        want = PO.estimate_normals_batch(frags, radius)
        _compare_normals("small shapes, radius %g" % radius, frags, got_n, got_c, want, 0.05)
        per = _split(fo, got_n)
        for b in (1, 2):                                                        # 1 and 2 points
            np.testing.assert_array_equal(per[b], np.tile([0.0, 0.0, 1.0], (b, 1)))
        np.testing.assert_array_equal(np.abs(per[PO.PLANAR]), np.tile([0.0, 0.0, 1.0], (64, 1)))   # exactly planar
        assert (_split(fo, got_c)[PO.PLANAR] >= 3).sum() >= 32
    # a fragment's normals do not depend on the fragments around it
    alone = FragmentOverlap([frags[-1]], "3DMatch", radius=PO.SMALL_R_INDEX)
    one_n, one_c = _raw_normals(alone, PO.SMALL_R_INDEX)
    assert one_n.tobytes() == per[-1].tobytes() and one_c.tobytes() == _split(fo, got_c)[-1].tobytes()


# ------------------------------------------------------------------------------------------------- fixed iterations
@pytest.mark.parametrize("max_dist", [0.075, 0.03])
def test_thirty_iterations_match_oracle_with_trace(gpu, max_dist):
    """max_dist 0.03 on the index of cell 0.075: the search ball is smaller than the cell"""
    got, want = _six(max_dist, 30, 0.0)
    assert all(w["iters"] == 30 and w["status"] == 0 for w in want)
    _compare(got, want)
    assert (got["trace"] >= 0).all()


def test_convergence_and_iteration_cap(gpu):
    """statuses 0 and 2 both occur: every pair converges within the 30 (4 to 12 solves), none within a cap of 3"""
    got, want = _six(0.075, 30, 1e-6)
    assert all(w["status"] == 0 and 0 < w["iters"] < 30 for w in want)
    _compare(got, want)
    for k, w in enumerate(want):                                        # -1 in the rows after the last evaluation
        assert (got["trace"][k][w["iters"] + 1:] == -1.0).all() and (got["trace"][k][:w["iters"] + 1] >= 0).all()
    got3, want3 = _six(0.075, 3, 1e-6)
    assert all(w["status"] == 2 and w["iters"] == 3 for w in want3)
    _compare(got3, want3)
    from lib.icp import icp_refine
    p2p = icp_refine(_fo(), O.SIX, _six_starts(), 0.075, 30)
    print("iterations to convergence at 1e-6: point-to-plane %s, point-to-point %s (status %s)"
          % ([w["iters"] for w in want], p2p["iters"].tolist(), p2p["status"].tolist()))


def test_full_copy_recovers_the_motion(gpu):
    from lib.overlap import FragmentOverlap
    from lib.icp import icp_refine
    src = O.scene4_centroids()[0]
    tgt, Tt, Ts = O.full_copy_case(src)
    fo = FragmentOverlap([src, tgt], "3DMatch", radius=0.075)
    fo.estimate_normals()                                                       # on the target with its distractors
    got = icp_refine(fo, [[0, 1]], Ts[None], 0.05, max_iters=10, tol_fitness=0.0, tol_rmse=0.0,
                     method="point_to_plane")
    print("|T - T_true| %.3g, rmse %.3g" % (np.abs(got["T"][0] - Tt).max(), got["rmse"][0]))
    np.testing.assert_allclose(got["T"][0], Tt, rtol=0, atol=TOL)
    assert got["n_corr"][0] == len(src) and got["fitness"][0] == 1.0 and got["iters"][0] == 10
    assert got["status"][0] == 0 and got["rmse"][0] < TOL


# ------------------------------------------------------------------------------------- small shapes and status bits
def _raw_call(fo, pairs, T0, max_dist, max_iters, tol):
    """mvr_icp_refine_plane on sentinel-filled output buffers -> numpy outputs"""
    import torch
    from lib import _native as N
    d = fo.device
    P = len(pairs)
    gp = torch.as_tensor(np.asarray(pairs, np.int64)).to(d)
    gT = torch.as_tensor(np.ascontiguousarray(np.asarray(T0, np.float64)[:, :3])).to(d)
    T = torch.full((P, 12), SENTINEL, dtype=torch.float64, device=d)
    fit, rm = (torch.full((P,), SENTINEL, dtype=torch.float64, device=d) for _ in range(2))
    nc, it, st = (torch.full((P,), int(SENTINEL), dtype=torch.int32, device=d) for _ in range(3))
    tr = torch.full((P, max_iters + 1, 2), SENTINEL, dtype=torch.float64, device=d)
    N.check(N.lib().mvr_icp_refine_plane(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.normals),
                                         N.ptr(fo.off_dev), fo.B, fo.M, fo.r, N.ptr(gp), N.ptr(gT), P, max_dist,
                                         max_iters, tol, tol, N.ptr(T), N.ptr(fit), N.ptr(rm), N.ptr(nc), N.ptr(it),
                                         N.ptr(st), N.ptr(tr), N.stream()), "mvr_icp_refine_plane")
    T4 = np.tile(np.eye(4), (P, 1, 1))
    T4[:, :3] = T.cpu().numpy().reshape(P, 3, 4)
    return {"T": T4, "fitness": fit.cpu().numpy(), "rmse": rm.cpu().numpy(), "n_corr": nc.cpu().numpy(),
            "iters": it.cpu().numpy(), "status": st.cpu().numpy(), "trace": tr.cpu().numpy()}


def test_small_shapes_and_status_bits_in_one_batch(gpu):
    from lib.overlap import FragmentOverlap
    frags, pairs, T0 = PO.corner_case()
    fo = FragmentOverlap(frags, "3DMatch", radius=PO.CORNER_RADIUS)
    fo.estimate_normals()
    nrm = _split(fo, fo.normals)
    np.testing.assert_array_equal(np.abs(nrm[1]), np.tile([0.0, 0.0, 1.0], (200, 1)))      # the planar target
    # two invalid pairs among the others: a NaN in T0 (with a payload), a fragment index B
    T_nan = T0[4].copy()
    T_nan[1, 2] = np.frombuffer(np.uint64(0x7FF8000000ABCDEF).tobytes(), np.float64)[0]
    pairs = np.concatenate([pairs[:3], [[6, 0]], pairs[3:6], [[len(frags), 0]], pairs[6:]])
    T0 = np.concatenate([T0[:3], T_nan[None], T0[3:6], T0[5:6], T0[6:]])
    want = PO.icp_plane_batch(frags, nrm, pairs, T0, PO.CORNER_RADIUS, 30, 0.0, 0.0)
    got = _raw_call(fo, pairs, T0, PO.CORNER_RADIUS, 30, 0.0)
    assert [w["status"] for w in want] == [1, 1, 1, 4, 0, 0, 0, 4, 0, 0, 1, 8]
    assert [w["n_corr"] for w in want][:5] == [0, 1, 5, 0, 6]
    for name in got:
        assert not np.any(got[name] == SENTINEL), name                  # every row of every output is written
    _compare(got, want)
    for k in (0, 1, 2, 10, 11):  # 0, 1, 5 correspondences, none at all, and the degenerate system: T = T0
        assert got["T"][k][:3].tobytes() == np.ascontiguousarray(T0[k][:3]).tobytes()
        assert got["iters"][k] == 0 and (got["trace"][k][1:] == -1.0).all()
    assert got["iters"][4] == 30 and not np.array_equal(got["T"][4][:3], T0[4][:3])        # 6: a solve happens
    assert got["n_corr"][11] >= 6 and got["fitness"][11] > 0 and got["trace"][11][0, 0] == got["fitness"][11]
    for k in (3, 7):             # invalid: T0 copied bit for bit, everything else 0, no evaluation in the trace
        assert got["T"][k][:3].tobytes() == np.ascontiguousarray(T0[k][:3]).tobytes()
        assert (got["fitness"][k], got["rmse"][k], got["n_corr"][k], got["iters"][k]) == (0.0, 0.0, 0, 0)
        assert (got["trace"][k] == -1.0).all()
    # the neighbours of the invalid pairs are what they are without them
    ok = [k for k in range(len(pairs)) if k not in (3, 7)]
    alone = _raw_call(fo, pairs[ok], T0[ok], PO.CORNER_RADIUS, 30, 0.0)
    for name in alone:
        assert alone[name].tobytes() == got[name][ok].tobytes(), name


# --------------------------------------------------------------------------------------------------- batch invariance
def test_outputs_do_not_depend_on_the_batch(gpu):
    from lib.icp import icp_refine
    fo = _fo()
    T6 = _six_starts()
    ref, _ = _six(0.075, 30, 0.0)
    kw = dict(max_dist=0.075, max_iters=30, tol_fitness=0.0, tol_rmse=0.0, return_trace=True, method="point_to_plane")

    def same(got, rows, where):
        for name in ref:
            assert np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(ref[name][rows]).tobytes(), \
                (where, name)

    for k in range(6):                                                  # each pair alone
        same(icp_refine(fo, [O.SIX[k]], T6[k:k + 1], **kw), [k], "alone %d" % k)
    perm = np.random.default_rng(1).permutation(6)                      # shuffled
    same(icp_refine(fo, np.asarray(O.SIX)[perm], T6[perm], **kw), perm, "shuffled")
    rows = np.array([0, 1, 2, 0, 1, 0, 5, 2, 2, 0, 0])                  # fragment 0 the source of several pairs
    same(icp_refine(fo, np.asarray(O.SIX)[rows], T6[rows], **kw), rows, "repeated")


def test_translation_invariance(gpu):
    """Every fragment moved by (100, -200, 50), the starts conjugated: T conjugated back agrees with the unshifted
    run within 1e-7 (a shift of 2e2 costs about 2e2 eps per coordinate and the loop is contractive).  The oracle's
    own shifted / unshifted difference on the CPU is 6.7e-14 (test_icp_plane_host.py), below 1e-9, so the bound
    stays 1e-7.  Without the per-pair origin c the cross products would carry the 2e2."""
    from lib.overlap import FragmentOverlap
    from lib.icp import icp_refine
    pts = _split(_fo(), _fo().xyz)
    T6 = _six_starts()
    kw = dict(max_dist=0.075, max_iters=30, tol_fitness=0.0, tol_rmse=0.0, method="point_to_plane")
    out = []
    for shift in (np.zeros(3), PO.SHIFT):
        fo = FragmentOverlap([p + shift for p in pts], "3DMatch", radius=0.075)
        fo.estimate_normals()
        got = icp_refine(fo, O.SIX, PO.conjugate_starts(T6, shift), **kw)
        assert (got["status"] == 0).all() and (got["iters"] == 30).all()
        out.append((PO.conjugate_starts(got["T"], -shift), got["n_corr"]))
    diff = np.abs(out[0][0] - out[1][0]).max()
    print("shifted by %s and conjugated back against unshifted: %.3g" % (PO.SHIFT.tolist(), diff))
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert diff <= 1e-7
    ref, _ = _six(0.075, 30, 0.0)                                       # the raw-point index holds the same points
    assert np.abs(out[0][0] - ref["T"]).max() <= TOL


# ----------------------------------------------------------------------------------------------------- Python surface
def test_python_surface_dtypes_and_devices(gpu):
    import torch
    from lib.icp import icp_refine, icp_pair
    from lib.overlap import FragmentOverlap
    fo = _fo()
    T6 = _six_starts()
    ref, _ = _six(0.075, 30, 1e-6)
    assert fo.normals.dtype == torch.float64 and fo.normals.device.type == "cuda" and fo.normals.shape == (fo.M, 3)
    assert fo.n_nbr.dtype == torch.int32 and fo.n_nbr.shape == (fo.M,)
    # fp64 torch on the device in -> torch on the device out, the same bits
    dev_out = icp_refine(fo, torch.tensor(O.SIX, device=gpu), torch.from_numpy(T6).to(gpu), 0.075, return_trace=True,
                         method="point_to_plane")
    assert all(torch.is_tensor(v) and v.device.type == "cuda" for v in dev_out.values())
    assert dev_out["T"].shape == (6, 4, 4) and dev_out["trace"].shape == (6, 31, 2)
    assert dev_out["n_corr"].dtype == torch.int32 and dev_out["T"].dtype == torch.float64
    for name in ref:
        assert dev_out[name].cpu().numpy().tobytes() == ref[name].tobytes(), name
    # [P,3,4] and fp32 inputs (torch on the host -> torch on the host, numpy -> numpy): the fp32 start, in fp64
    T32 = T6[:, :3].astype(np.float32)
    want = icp_refine(fo, O.SIX, T32.astype(np.float64), 0.075, method="point_to_plane")
    for Tin in (torch.from_numpy(T32), T32):
        out = icp_refine(fo, O.SIX, Tin, 0.075, method="point_to_plane")
        assert all((torch.is_tensor(v) and v.device.type == "cpu") if torch.is_tensor(Tin) else
                   isinstance(v, np.ndarray) for v in out.values()) and "trace" not in out
        for name in want:
            assert np.asarray(out[name]).tobytes() == want[name].tobytes(), name
    # the default method is the point-to-point loop, the same bytes as a call that omits it
    plain = icp_refine(fo, O.SIX, T6, 0.075, return_trace=True)
    named = icp_refine(fo, O.SIX, T6, 0.075, return_trace=True, method="point_to_point")
    for name in plain:
        assert plain[name].tobytes() == named[name].tobytes(), name
    assert not np.array_equal(plain["T"], ref["T"])
    # without normals: an error, also after the caller's own normals of another shape
    bare = FragmentOverlap(O.scene4()[0][:2], "FCGF", 0.025)
    with pytest.raises(ValueError, match="normals"):
        icp_refine(bare, [[0, 1]], T6[:1], method="point_to_plane")
    bare.normals = fo.normals
    with pytest.raises(ValueError, match="normals"):
        icp_refine(bare, [[0, 1]], T6[:1], method="point_to_plane")
    with pytest.raises(ValueError):
        bare.estimate_normals(radius=0.08)
    # a caller's own normals: the two fragments' rows of the scene's (the same centroids in the same order)
    bare.normals = fo.normals[:bare.M].clone()
    own = icp_refine(bare, [[0, 1]], T6[:1], 0.075, method="point_to_plane")
    assert own["T"].tobytes() == ref["T"][:1].tobytes()
    # icp_pair: estimates the normals itself, on an index of cell max(max_dist, normal_radius)
    src, tgt, T_one, max_dist, iters = O.pair_case()
    one = icp_pair(src, tgt, T_one, max_dist=max_dist, max_iters=iters, method="point_to_plane", normal_radius=0.09)
    fo2 = FragmentOverlap([src, tgt], "3DMatch", radius=0.09)
    nrm = _split(fo2, fo2.estimate_normals(0.09))
    w = PO.icp_plane(src, tgt, nrm[1], T_one, max_dist, iters)
    assert one["T"].shape == (4, 4) and int(one["n_corr"]) == w["n_corr"] and int(one["iters"]) == w["iters"]
    assert int(one["status"]) == w["status"]
    assert np.abs(one["T"][:3] - w["T"]).max() <= TOL and abs(one["rmse"] - w["rmse"]) <= TOL
    p2p = icp_pair(src, tgt, T_one, max_dist=max_dist, max_iters=iters)
    assert p2p["T"].tobytes() == icp_pair(src, tgt, T_one, max_dist=max_dist, max_iters=iters,
                                          method="point_to_point")["T"].tobytes()


# ------------------------------------------------------------------------------------------------------------ harness
def test_benchmark_harness_with_point_to_plane_icp(gpu, tmp_path):
    """--icp --icp_method point_to_plane refines every pair's estimate on the batch's FragmentOverlap and its normals
    before the inversion: every written transform equals inv(icp_refine(., method='point_to_plane')) of the run
    without the flag; the default method writes what --icp alone writes."""
    import shutil
    from eval_layout import write_scene, read_results
    from lib.icp import icp_refine
    from lib.overlap import FragmentOverlap
    from lib.utils import read_trajectory
    from scripts.benchmark_pairwise_registration import main
    roots = [str(tmp_path / n) for n in ("plain", "plane", "p2p", "p2p_named")]
    pairs = write_scene(os.path.join(roots[0], "3d_match"), "kitchen", 4, 600, seed=0)
    for r in roots[1:]:
        shutil.copytree(roots[0], r)
    argv = ["--method", "RANSAC", "--batch_size", "4", "--num_workers", "0"]
    main(["--source_path", roots[0]] + argv)
    s1 = main(["--source_path", roots[1]] + argv + ["--icp", "--icp_iters", "20", "--icp_method", "point_to_plane",
                                                    "--icp_normal_radius", "0.06"])
    s2 = main(["--source_path", roots[2]] + argv + ["--icp", "--icp_iters", "20"])
    s3 = main(["--source_path", roots[3]] + argv + ["--icp", "--icp_iters", "20", "--icp_method", "point_to_point"])
    assert read_results(roots[2], "3d_match", "RANSAC") == read_results(roots[3], "3d_match", "RANSAC") and s2 == s3
    assert s1["recall"] == 1.0 and s1["precision"] == 1.0
    for bad in (["--icp_normal_radius", "0.08"], ["--icp_normal_radius", "0"]):
        with pytest.raises(ValueError):
            main(["--source_path", roots[1]] + argv + ["--icp", "--icp_method", "point_to_plane"] + bad)
    traj = []
    for r in roots[:2]:
        keys, t = read_trajectory(os.path.join(r, "3d_match", "results", "RANSAC", "all", "kitchen", "traj.txt"))
        assert keys.tolist() == [[str(i), str(j), "True"] for i, j in pairs] and t.shape == (6, 4, 4)
        traj.append(t)
    clouds = [np.load(os.path.join(roots[0], "3d_match", "features", "kitchen", "kitchen_%03d.npz" % k))["xyz"]
              for k in range(4)]
    fo = FragmentOverlap(clouds, "FCGF")
    fo.estimate_normals(0.06)
    ref = icp_refine(fo, pairs, np.linalg.inv(traj[0]), max_iters=20, method="point_to_plane")
    print("refined vs plain: %.3g; written vs inv(icp_refine): %.3g; iters %s, status %s"
          % (np.abs(traj[1] - traj[0]).max(), np.abs(traj[1] - np.linalg.inv(ref["T"])).max(), ref["iters"].tolist(),
             ref["status"].tolist()))
    # the files hold 12 decimals and the refinement restarts from them: the scene's fragments are exact copies, so
    # the loop lands on the same fixed point from either start
    np.testing.assert_allclose(traj[1], np.linalg.inv(ref["T"]), rtol=0, atol=1e-9)
    assert not np.array_equal(traj[1], traj[0])
