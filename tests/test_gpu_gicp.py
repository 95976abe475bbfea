"""GPU generalized (plane-to-plane) ICP (csrc/icp_gicp.hip mvr_icp_refine_generalized, lib/icp.py gicp_refine /
gicp_pair) against the numpy / sklearn oracle (tests/gicp_oracle.py): fixed iteration counts with the full trace,
convergence, the covariance parameter, the status bits on small and awkward shapes, a degenerate system, batch, sign
and translation invariance, the Python surface and the benchmark harness's --icp_method generalized.

Tolerance: 1e-9 on T, fitness, rmse and the trace (the project's fp64 bound; largest difference seen on an MI355X
2.5e-15, at cond(H) up to 9.6e3 and cond(M) up to 1e3); n_corr, iters and status exactly.  The
comparisons feed the oracle the GPU's own points and normals, so the normals' sign and eigen-solver rounding stay out
of them.  test_gicp_host.py checks that no case used here has a correspondence, a stopping test or a pivot test within
rounding of a tie."""
import functools
import os
import sys

import numpy as np
import pytest

import icp_oracle as O
import icp_plane_oracle as PO
import gicp_oracle as GO

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
if HELPERS not in sys.path:
    sys.path.insert(0, HELPERS)

pytestmark = pytest.mark.gpu
TOL = 1e-9
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
def _six(max_dist, max_iters, tol, epsilon=GO.EPSILON):
    """(GPU result with trace, oracle results on the GPU's points and normals) of the six pairs"""
    from lib.icp import gicp_refine
    fo = _fo()
    got = gicp_refine(fo, O.SIX, _six_starts(), max_dist, max_iters, tol, tol, epsilon, return_trace=True)
    nrm = _split(fo, fo.normals)
    want = GO.gicp_batch(_split(fo, fo.xyz), nrm, O.SIX, _six_starts(), max_dist, max_iters, tol, tol, epsilon)
    return got, want


def _compare(got, want, trace=True):
    worst = 0.0
    for k, w in enumerate(want):
        for name in ("n_corr", "iters", "status"):
            assert int(got[name][k]) == w[name], (k, name, int(got[name][k]), w[name])
        if w["status"] & 4:      # T0 (possibly not finite) copied bit for bit
            assert got["T"][k][:3].tobytes() == np.ascontiguousarray(w["T"]).tobytes(), k
        dT = 0.0 if w["status"] & 4 else np.abs(got["T"][k][:3] - w["T"]).max()
        df, dr = abs(got["fitness"][k] - w["fitness"]), abs(got["rmse"][k] - w["rmse"])
        dtr = np.abs(got["trace"][k] - w["trace"]).max() if trace else 0.0
        print("pair %d: |dT| %.3g, |d fitness| %.3g, |d rmse| %.3g, |d trace| %.3g, iters %d, status %d, cond(H) %.3g"
              % (k, dT, df, dr, dtr, w["iters"], w["status"], max(w["cond"] + [0.0])))
        worst = max(worst, dT, df, dr, dtr)
        assert dT <= TOL and df <= TOL and dr <= TOL and dtr <= TOL, k
        np.testing.assert_array_equal(got["T"][k][3], [0.0, 0.0, 0.0, 1.0])
    print("largest difference against the oracle: %.3g" % worst)


# ------------------------------------------------------------------------------------------------- fixed iterations
@pytest.mark.parametrize("max_dist", [0.075, 0.03])
def test_thirty_iterations_match_oracle_with_trace(gpu, max_dist):
    """max_dist 0.03 on the index of cell 0.075: the search ball is smaller than the cell"""
    got, want = _six(max_dist, 30, 0.0)
    assert all(w["iters"] == 30 and w["status"] == 0 for w in want)
    _compare(got, want)
    assert (got["trace"] >= 0).all()


@pytest.mark.parametrize("epsilon", [1.0, 1e-2])
def test_other_epsilons_match_oracle(gpu, epsilon):
    got, want = _six(0.075, 30, 0.0, epsilon)
    assert all(w["iters"] == 30 and w["status"] == 0 for w in want)
    _compare(got, want)
    assert not np.array_equal(got["T"], _six(0.075, 30, 0.0)[0]["T"])            # the parameter reaches the kernel


def test_convergence_and_iteration_cap(gpu):
    """statuses 0 and 2 both occur: every pair converges within the 30 (4 to 5 solves), none within a cap of 3"""
    got, want = _six(0.075, 30, 1e-6)
    assert all(w["status"] == 0 and 0 < w["iters"] < 30 for w in want)
    _compare(got, want)
    for k, w in enumerate(want):                                        # -1 in the rows after the last evaluation
        assert (got["trace"][k][w["iters"] + 1:] == -1.0).all() and (got["trace"][k][:w["iters"] + 1] >= 0).all()
    got3, want3 = _six(0.075, 3, 1e-6)
    assert all(w["status"] == 2 and w["iters"] == 3 for w in want3)
    _compare(got3, want3)
    print("iterations to convergence at 1e-6: generalized %s" % [w["iters"] for w in want])


def test_error_against_ground_truth_is_below_point_to_plane(gpu):
    from lib.icp import icp_refine
    poses = O.scene4()[1]
    gt = np.asarray([O.gt_transform(poses, i, j) for i, j in O.SIX])
    gen = _six(0.075, 30, 0.0)[0]
    p2l = icp_refine(_fo(), O.SIX, _six_starts(), 0.075, 30, 0.0, 0.0, method="point_to_plane")
    e_gen, e_p2l = np.abs(gen["T"] - gt).max(), np.abs(p2l["T"] - gt).max()
    print("largest |T - T_gt| after 30 iterations: generalized %.3g, point-to-plane %.3g" % (e_gen, e_p2l))
    assert e_gen < e_p2l


# ------------------------------------------------------------------------------------- small shapes and status bits
def _raw_call(fo, pairs, T0, max_dist, max_iters, tol, epsilon=GO.EPSILON):
    """mvr_icp_refine_generalized on sentinel-filled output buffers -> numpy outputs"""
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
    N.check(N.lib().mvr_icp_refine_generalized(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.normals),
                                               N.ptr(fo.off_dev), fo.B, fo.M, fo.r, N.ptr(gp), N.ptr(gT), P, max_dist,
                                               epsilon, max_iters, tol, tol, N.ptr(T), N.ptr(fit), N.ptr(rm),
                                               N.ptr(nc), N.ptr(it), N.ptr(st), N.ptr(tr), N.stream()),
            "mvr_icp_refine_generalized")
    T4 = np.tile(np.eye(4), (P, 1, 1))
    T4[:, :3] = T.cpu().numpy().reshape(P, 3, 4)
    return {"T": T4, "fitness": fit.cpu().numpy(), "rmse": rm.cpu().numpy(), "n_corr": nc.cpu().numpy(),
            "iters": it.cpu().numpy(), "status": st.cpu().numpy(), "trace": tr.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def _corner():
    """(index with normals over 0.1, frags, pairs, T0, row of the line pair) of corner_case() plus the line source"""
    from lib.overlap import FragmentOverlap
    frags, pairs, T0, line = GO.line_case()
    fo = FragmentOverlap(frags, "3DMatch", radius=PO.CORNER_RADIUS)
    fo.estimate_normals()
    return fo, frags, pairs, T0, line


@pytest.mark.parametrize("epsilon", [GO.EPSILON, 1.0])
def test_small_shapes_status_bits_and_the_degenerate_line(gpu, epsilon):
    fo, frags, pairs, T0, line = _corner()
    nrm = _split(fo, fo.normals)
    np.testing.assert_allclose(np.linalg.norm(np.concatenate(nrm), axis=1), 1.0, rtol=0, atol=1e-14)
    want = GO.gicp_batch(frags, nrm, pairs, T0, GO.LINE_MAX_DIST, 30, 0.0, 0.0, epsilon)
    got = _raw_call(fo, pairs, T0, GO.LINE_MAX_DIST, 30, 0.0, epsilon)
    # sources of 0, 1, 5, 6, 63, 64, 65, 1025 points, the far one, the one against the planar target, the line
    assert [w["status"] for w in want] == [1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 8]
    assert [w["n_corr"] for w in want][:4] == [0, 1, 5, 6]
    for name in got:
        assert not np.any(got[name] == SENTINEL), name                  # every row of every output is written
    _compare(got, want)
    for k in (0, 1, 2, 8, line):     # 0, 1, 5 correspondences, none at all, and the degenerate system: T = T0
        assert got["T"][k][:3].tobytes() == np.ascontiguousarray(T0[k][:3]).tobytes()
        assert got["iters"][k] == 0 and (got["trace"][k][1:] == -1.0).all()
    assert got["status"][line] == 8 and got["n_corr"][line] == 9 and got["fitness"][line] == 1.0
    assert got["trace"][line][0, 0] == 1.0
    assert got["iters"][3] == 30 and not np.array_equal(got["T"][3][:3], T0[3][:3])        # 6: a solve happens
    assert got["iters"][9] == 30 and got["status"][9] == 0             # the planar target is no degeneracy here


def test_invalid_pairs(gpu):
    fo, frags, pairs, T0, line = _corner()
    # two invalid pairs among the others: a NaN in T0 (with a payload), a fragment index B
    T_nan = T0[4].copy()
    T_nan[1, 2] = np.frombuffer(np.uint64(0x7FF8000000ABCDEF).tobytes(), np.float64)[0]
    T_inf = T0[5].copy()
    T_inf[0, 3] = np.inf
    pairs2 = np.concatenate([pairs[:3], [[6, 0]], pairs[3:6], [[len(frags), 0]], [[7, 0]], [[-1, 0]], pairs[6:]])
    T02 = np.concatenate([T0[:3], T_nan[None], T0[3:6], T0[5:6], T_inf[None], T0[5:6], T0[6:]])
    bad = (3, 7, 8, 9)
    want = GO.gicp_batch(frags, _split(fo, fo.normals), pairs2, T02, GO.LINE_MAX_DIST, 30, 0.0, 0.0)
    got = _raw_call(fo, pairs2, T02, GO.LINE_MAX_DIST, 30, 0.0)
    assert [w["status"] for w in want] == [1, 1, 1, 4, 0, 0, 0, 4, 4, 4, 0, 0, 1, 0, 8]
    for name in got:
        assert not np.any(got[name] == SENTINEL), name
    _compare(got, want)
    for k in bad:                # T0 copied bit for bit, everything else 0, no evaluation in the trace
        assert got["status"][k] == 4
        assert got["T"][k][:3].tobytes() == np.ascontiguousarray(T02[k][:3]).tobytes()
        assert (got["fitness"][k], got["rmse"][k], got["n_corr"][k], got["iters"][k]) == (0.0, 0.0, 0, 0)
        assert (got["trace"][k] == -1.0).all()
    # the neighbours of the invalid pairs are what they are without them
    ok = [k for k in range(len(pairs2)) if k not in bad]
    alone = _raw_call(fo, pairs2[ok], T02[ok], GO.LINE_MAX_DIST, 30, 0.0)
    for name in alone:
        assert alone[name].tobytes() == got[name][ok].tobytes(), name


def test_four_entries_share_one_search(gpu):
    """One evaluation (max_iters 0) of small_normals_case's fragments of 0, 1, 2, 3, 63, 64, 65 and 1025 points: the
    three refinements and information_matrix count the same correspondences, and their rmse (and the refinements'
    fitness) is the same bit for bit.  The per-thread summands of n and sum d^2 are the same in the same order, and
    block_sum reduces each component independently of how many there are."""
    from lib.icp import gicp_refine, icp_refine, information_matrix
    from lib.overlap import FragmentOverlap
    fo = FragmentOverlap(PO.small_normals_case(), "3DMatch", radius=PO.SMALL_R_INDEX)
    fo.estimate_normals()
    pairs, T0 = PO.small_normals_pairs()
    kw = dict(max_iters=0, tol_fitness=0.0, tol_rmse=0.0)
    got = [icp_refine(fo, pairs, T0, method=m, **kw) for m in ("point_to_point", "point_to_plane")] + \
        [gicp_refine(fo, pairs, T0, **kw), information_matrix(fo, pairs, T0)]
    ref = got[0]
    print("n_corr %s\nrmse %s" % (ref["n_corr"].tolist(), ref["rmse"].tolist()))
    assert (ref["status"] == 0).all() and (ref["iters"] == 0).all()
    big = len(PO.SMALL_SIZES) - 1                # sources 0..big against the cloud, then the cloud against targets 0..
    assert ref["n_corr"][big] == 1025 and ref["n_corr"][0] == 0 and ref["n_corr"][big + 1] == 0
    assert (ref["n_corr"][1:big] == PO.SMALL_SIZES[1:big]).all() and (ref["n_corr"][big + 2:] > 0).all()
    assert ((ref["rmse"] > 0) == (ref["n_corr"] > 0)).all()
    for other in got[1:]:
        np.testing.assert_array_equal(other["n_corr"], ref["n_corr"])
        assert other["rmse"].tobytes() == ref["rmse"].tobytes()
        if "fitness" in other:
            assert other["fitness"].tobytes() == ref["fitness"].tobytes()


@pytest.mark.parametrize("radius", [0.06, PO.SMALL_R_INDEX])
def test_per_point_entries_share_one_walk(gpu, radius):
    """The entries that walk a point's ball on the index (csrc/rindex.hpp ball_walk), on small_normals_case's
    fragments of 0, 1, 2, 3, 63, 64, 65 and 1025 points at a radius inside the cell and at exactly the cell: the
    neighbour counts of mvr_estimate_normals, mvr_iss_saliency, mvr_color_gradient and mvr_radius_count are the
    oracle's, element for element; a point alone in its ball has an all-zero SPFH row; and the seven entries write
    every row of every output, the neighbours of the empty fragment included."""
    import point_entries
    from lib import _native as N
    frags = PO.small_normals_case()
    out = {k: v.cpu().numpy() for k, v in point_entries.run(gpu, N.lib(), frags, PO.SMALL_R_INDEX, radius,
                                                            ks=(20,)).items()}
    want = np.concatenate([f["n_nbr"] for f in PO.estimate_normals_batch(frags, radius)])
    print("radius %g: counts %d..%d, %d points alone" % (radius, want.min(), want.max(), (want == 1).sum()))
    assert want.min() == 1 and want.max() > 50     # no distance is within 1e-7 of either radius: counts are exact
    for name in ("normals n_nbr", "normals vp n_nbr", "iss n_nbr", "color n_nbr", "count count"):
        np.testing.assert_array_equal(out[name], want, err_msg=name)
    assert not out["fpfh spfh"][want == 1].any()
    for name, x in out.items():
        if not name.startswith("stat "):
            sent = point_entries.SENT & 0xff if x.dtype == np.uint8 else point_entries.SENT
            assert not (x == sent).any(), name


# -------------------------------------------------------------------------------------------------------- invariances
def test_outputs_do_not_depend_on_the_batch(gpu):
    from lib.icp import gicp_refine
    fo = _fo()
    T6 = _six_starts()
    ref, _ = _six(0.075, 30, 0.0)
    kw = dict(max_dist=0.075, max_iters=30, tol_fitness=0.0, tol_rmse=0.0, return_trace=True)

    def same(got, rows, where):
        for name in ref:
            assert np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(ref[name][rows]).tobytes(), \
                (where, name)

    for k in range(6):                                                  # each pair alone
        same(gicp_refine(fo, [O.SIX[k]], T6[k:k + 1], **kw), [k], "alone %d" % k)
    perm = np.random.default_rng(1).permutation(6)                      # shuffled
    same(gicp_refine(fo, np.asarray(O.SIX)[perm], T6[perm], **kw), perm, "shuffled")
    rows = np.array([0, 1, 2, 0, 1, 0, 5, 2, 2, 0, 0])                  # fragment 0 the source of several pairs
    same(gicp_refine(fo, np.asarray(O.SIX)[rows], T6[rows], **kw), rows, "repeated")


def test_negated_normals_agree(gpu):
    """only n n^T and m m^T enter, so the sign of a normal cannot matter: required within TOL, bit-identity reported"""
    from lib.icp import gicp_refine
    fo = _fo()
    ref, _ = _six(0.075, 30, 0.0)
    keep = fo.normals
    try:
        fo.normals = (-keep).contiguous()
        neg = gicp_refine(fo, O.SIX, _six_starts(), 0.075, 30, 0.0, 0.0, return_trace=True)
    finally:
        fo.normals = keep
    diff = max(np.abs(neg[name].astype(np.float64) - ref[name]).max() for name in ref)
    print("all normals negated: largest difference %.3g, bit-identical %s"
          % (diff, all(neg[name].tobytes() == ref[name].tobytes() for name in ref)))
    for name in ("n_corr", "iters", "status"):
        np.testing.assert_array_equal(neg[name], ref[name])
    assert diff <= TOL


def test_translation_invariance(gpu):
    """Every fragment moved by (100, -200, 50), the starts conjugated: T conjugated back agrees with the unshifted run
    within TOL.  A shift of 2e2 costs about 2e2 eps = 4e-14 per coordinate, cond(H) <= 1.7e3 and the loop is
    contractive; the oracle's own shifted / unshifted difference is 5.7e-14 (test_gicp_host.py).  Without the per-pair
    origin c the cross products would carry the 2e2."""
    from lib.overlap import FragmentOverlap
    from lib.icp import gicp_refine
    pts = _split(_fo(), _fo().xyz)
    T6 = _six_starts()
    kw = dict(max_dist=0.075, max_iters=30, tol_fitness=0.0, tol_rmse=0.0)
    out = []
    for shift in (np.zeros(3), PO.SHIFT):
        fo = FragmentOverlap([p + shift for p in pts], "3DMatch", radius=0.075)
        fo.estimate_normals()
        got = gicp_refine(fo, O.SIX, PO.conjugate_starts(T6, shift), **kw)
        assert (got["status"] == 0).all() and (got["iters"] == 30).all()
        out.append((PO.conjugate_starts(got["T"], -shift), got["n_corr"]))
    diff = np.abs(out[0][0] - out[1][0]).max()
    print("shifted by %s and conjugated back against unshifted: %.3g" % (PO.SHIFT.tolist(), diff))
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert diff <= TOL
    ref, _ = _six(0.075, 30, 0.0)                                       # the raw-point index holds the same points
    assert np.abs(out[0][0] - ref["T"]).max() <= TOL


# ----------------------------------------------------------------------------------------------------- Python surface
def test_python_surface_dtypes_and_devices(gpu):
    import torch
    from lib.icp import gicp_refine, gicp_pair, icp_refine
    from lib.overlap import FragmentOverlap
    fo = _fo()
    T6 = _six_starts()
    ref, _ = _six(0.075, 30, 1e-6)
    assert all(isinstance(v, np.ndarray) for v in ref.values())                  # numpy in, numpy out
    # fp64 torch on the device in -> torch on the device out, the same bits
    dev_out = gicp_refine(fo, torch.tensor(O.SIX, device=gpu), torch.from_numpy(T6).to(gpu), 0.075, return_trace=True)
    assert all(torch.is_tensor(v) and v.device.type == "cuda" for v in dev_out.values())
    assert dev_out["T"].shape == (6, 4, 4) and dev_out["trace"].shape == (6, 31, 2)
    assert dev_out["n_corr"].dtype == torch.int32 and dev_out["T"].dtype == torch.float64
    for name in ref:
        assert dev_out[name].cpu().numpy().tobytes() == ref[name].tobytes(), name
    # [P,3,4] and fp32 inputs (torch on the host -> torch on the host, numpy -> numpy): the fp32 start, in fp64
    T32 = T6[:, :3].astype(np.float32)
    want = gicp_refine(fo, O.SIX, T32.astype(np.float64), 0.075)
    for Tin in (torch.from_numpy(T32), T32):
        out = gicp_refine(fo, O.SIX, Tin, 0.075)
        assert all((torch.is_tensor(v) and v.device.type == "cpu") if torch.is_tensor(Tin) else
                   isinstance(v, np.ndarray) for v in out.values()) and "trace" not in out
        for name in want:
            assert np.asarray(out[name]).tobytes() == want[name].tobytes(), name
    # another loop than the other two methods'
    for method in ("point_to_point", "point_to_plane"):
        assert not np.array_equal(icp_refine(fo, O.SIX, T6, 0.075, method=method)["T"], ref["T"])
    # without normals: an error, also after the caller's own normals of another shape
    bare = FragmentOverlap(O.scene4()[0][:2], "FCGF", 0.025)
    with pytest.raises(ValueError, match="normals"):
        gicp_refine(bare, [[0, 1]], T6[:1])
    bare.normals = fo.normals
    with pytest.raises(ValueError, match="normals"):
        gicp_refine(bare, [[0, 1]], T6[:1])
    # a caller's own normals: the two fragments' rows of the scene's (the same centroids in the same order)
    bare.normals = fo.normals[:bare.M].clone()
    own = gicp_refine(bare, [[0, 1]], T6[:1], 0.075)
    assert own["T"].tobytes() == ref["T"][:1].tobytes()
    # gicp_pair: estimates both clouds' normals itself, on an index of cell max(max_dist, normal_radius); the same
    # bits as gicp_refine on such an index, and the oracle's result
    src, tgt, T_one, max_dist, iters = O.pair_case()
    one = gicp_pair(src, tgt, T_one, max_dist=max_dist, max_iters=iters, normal_radius=0.09, return_trace=True)
    fo2 = FragmentOverlap([src, tgt], "3DMatch", radius=0.09)
    nrm = _split(fo2, fo2.estimate_normals(0.09))
    by_hand = gicp_refine(fo2, [[0, 1]], T_one[None], max_dist, max_iters=iters, return_trace=True)
    for name in by_hand:
        assert one[name].tobytes() == by_hand[name][0].tobytes(), name
    w = GO.gicp(src, tgt, nrm[0], nrm[1], T_one, max_dist, iters)
    assert one["T"].shape == (4, 4) and one["trace"].shape == (iters + 1, 2)
    assert int(one["n_corr"]) == w["n_corr"] and int(one["iters"]) == w["iters"] and int(one["status"]) == w["status"]
    assert np.abs(one["T"][:3] - w["T"]).max() <= TOL and abs(one["rmse"] - w["rmse"]) <= TOL


# ------------------------------------------------------------------------------------------------------------ harness
def test_benchmark_harness_with_generalized_icp(gpu, tmp_path):
    """--icp --icp_method generalized refines every pair's estimate on the batch's FragmentOverlap and its normals
    before the inversion: every written transform equals inv(gicp_refine(.)) of the run without the flag."""
    import shutil
    from eval_layout import write_scene
    from lib.icp import gicp_refine
    from lib.overlap import FragmentOverlap
    from lib.utils import read_trajectory
    from scripts.benchmark_pairwise_registration import main
    roots = [str(tmp_path / n) for n in ("plain", "gicp")]
    pairs = write_scene(os.path.join(roots[0], "3d_match"), "kitchen", 4, 600, seed=0)
    shutil.copytree(roots[0], roots[1])
    argv = ["--method", "RANSAC", "--batch_size", "4", "--num_workers", "0"]
    gen = ["--icp", "--icp_iters", "20", "--icp_method", "generalized", "--icp_normal_radius", "0.06"]
    for bad in (["--icp_gicp_epsilon", "0"], ["--icp_gicp_epsilon", "1.5"], ["--icp_gicp_epsilon", "nan"],
                ["--icp_normal_radius", "0.08"]):
        with pytest.raises(ValueError):
            main(["--source_path", roots[1]] + argv + gen + bad)
    main(["--source_path", roots[0]] + argv)
    s1 = main(["--source_path", roots[1]] + argv + gen + ["--icp_gicp_epsilon", "0.01"])
    assert s1["recall"] == 1.0 and s1["precision"] == 1.0
    traj = []
    for r in roots:
        keys, t = read_trajectory(os.path.join(r, "3d_match", "results", "RANSAC", "all", "kitchen", "traj.txt"))
        assert keys.tolist() == [[str(i), str(j), "True"] for i, j in pairs] and t.shape == (6, 4, 4)
        traj.append(t)
    clouds = [np.load(os.path.join(roots[0], "3d_match", "features", "kitchen", "kitchen_%03d.npz" % k))["xyz"]
              for k in range(4)]
    fo = FragmentOverlap(clouds, "FCGF")
    fo.estimate_normals(0.06)
    ref = gicp_refine(fo, pairs, np.linalg.inv(traj[0]), max_iters=20, epsilon=0.01)
    print("refined vs plain: %.3g; written vs inv(gicp_refine): %.3g; iters %s, status %s"
          % (np.abs(traj[1] - traj[0]).max(), np.abs(traj[1] - np.linalg.inv(ref["T"])).max(), ref["iters"].tolist(),
             ref["status"].tolist()))
    # the files hold 12 decimals and the refinement restarts from them: the scene's fragments are exact copies, so
    # the loop lands on the same fixed point from either start
    np.testing.assert_allclose(traj[1], np.linalg.inv(ref["T"]), rtol=0, atol=1e-9)
    assert not np.array_equal(traj[1], traj[0])
