"""GPU ICP refinement (csrc/icp.hip mvr_icp_refine, lib/icp.py) against the numpy / sklearn oracle
(tests/icp_oracle.py): evaluation only (the correspondence counts pinned to the overlap gate's, which is itself tested
against sklearn), fixed iteration counts with the full trace, convergence, ground truth, small and awkward shapes,
invalid pairs, batch invariance bit for bit, the Python surface and the benchmark harness's --icp.

Tolerance: 1e-9 on T, fitness, rmse and the trace, the project's fp64 bound (the Procrustes f64 and synchronisation
tests); n_corr, iters and status exactly.  test_icp_host.py checks that no case used here has a nearest-neighbour
choice, a max_dist test or a stopping test within rounding of a tie."""
import functools
import os
import sys

import numpy as np
import pytest

import icp_oracle as O

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
if HELPERS not in sys.path:
    sys.path.insert(0, HELPERS)

pytestmark = pytest.mark.gpu
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def _fo(method, radius=None):
    from lib.overlap import FragmentOverlap
    return FragmentOverlap(O.scene4()[0], method, 0.025, radius=radius)


def _points(fo):
    """the fragments as the index holds them (for 'FCGF' the centroids in the GPU's row order)"""
    xyz = fo.xyz.cpu().numpy()
    return [xyz[fo.off[b]:fo.off[b + 1]] for b in range(fo.B)]


@functools.lru_cache(maxsize=None)
def _six_starts():
    return O.scene4_starts(O.SIX, O.scene4_centroids())


@functools.lru_cache(maxsize=None)
def _six(max_dist, max_iters, tol):
    """(GPU result with trace, oracle results) of the six pairs on the centroid index"""
    from lib.icp import icp_refine
    fo = _fo("FCGF")
    got = icp_refine(fo, O.SIX, _six_starts(), max_dist, max_iters, tol, tol, return_trace=True)
    return got, O.icp_batch(_points(fo), O.SIX, _six_starts(), max_dist, max_iters, tol, tol)


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


# --------------------------------------------------------------------------------------------------- evaluation only
@pytest.mark.parametrize("method", ["FCGF", "3DMatch"])
def test_evaluation_only_matches_overlap_counts_and_oracle(gpu, method):
    from lib.icp import icp_refine
    fo = _fo(method)
    assert fo.r == (3 * 0.025 if method == "FCGF" else 0.05)          # radius left at the method's default
    frags = _points(fo)
    T = O.eval_starts(O.scene4_centroids() if method == "FCGF" else O.scene4()[0])
    got = icp_refine(fo, O.TWELVE, T, max_iters=0, return_trace=True)
    # (i, j) rows: the pc_i column of counts with trans = inv(T); (j, i) rows: the pc_j column with trans = T
    c_ij = fo.counts(O.SIX, np.linalg.inv(T[:6]))[:, 0]
    c_ji = fo.counts(O.SIX, T[6:])[:, 1]
    np.testing.assert_array_equal(got["n_corr"], np.concatenate([c_ij, c_ji]))
    assert got["n_corr"].min() > 500 and len(set(got["n_corr"].tolist())) > 6
    np.testing.assert_array_equal(got["T"][:, :3], T[:, :3])          # no solve: T0 comes back
    _compare(got, O.icp_batch(frags, O.TWELVE, T, fo.r, 0))


# ------------------------------------------------------------------------------------------------- fixed iterations
@pytest.mark.parametrize("max_dist", [0.075, 0.03])
def test_thirty_iterations_match_oracle_with_trace(gpu, max_dist):
    """max_dist 0.03 on the index of cell 0.075: the search ball is smaller than the cell"""
    got, want = _six(max_dist, 30, 0.0)
    assert all(w["iters"] == 30 and w["status"] == 0 for w in want)
    _compare(got, want)
    assert (got["trace"] >= 0).all()


def test_convergence_and_iteration_cap(gpu):
    got, want = _six(0.075, 30, 1e-6)
    assert sorted(set(w["status"] for w in want)) == [0, 2] and min(w["iters"] for w in want) < 30
    _compare(got, want)
    for k, w in enumerate(want):                                        # -1 in the rows after the last evaluation
        assert (got["trace"][k][w["iters"] + 1:] == -1.0).all() and (got["trace"][k][:w["iters"] + 1] >= 0).all()
    got3, want3 = _six(0.075, 3, 1e-6)
    assert all(w["status"] == 2 and w["iters"] == 3 for w in want3)
    _compare(got3, want3)


def test_full_copy_recovers_the_motion(gpu):
    from lib.overlap import FragmentOverlap
    from lib.icp import icp_refine
    src = O.scene4_centroids()[0]
    tgt, Tt, Ts = O.full_copy_case(src)
    for max_dist in (0.025, 0.05):
        fo = FragmentOverlap([src, tgt], "3DMatch", radius=max_dist)
        got = icp_refine(fo, [[0, 1]], Ts[None], max_iters=10, tol_fitness=0.0, tol_rmse=0.0)
        print("max_dist %g: |T - T_true| %.3g, rmse %.3g" % (max_dist, np.abs(got["T"][0] - Tt).max(), got["rmse"][0]))
        np.testing.assert_allclose(got["T"][0], Tt, rtol=0, atol=TOL)
        assert got["n_corr"][0] == len(src) and got["fitness"][0] == 1.0 and got["iters"][0] == 10
        assert got["status"][0] == 0 and got["rmse"][0] < TOL


# ------------------------------------------------------------------------------------------ small and awkward shapes
def _raw_call(fo, pairs, T0, max_dist, max_iters, tol, sentinel=-77.0):
    """mvr_icp_refine on sentinel-filled output buffers -> numpy outputs"""
    import torch
    from lib import _native as N
    d = fo.device
    P = len(pairs)
    gp = torch.as_tensor(np.asarray(pairs, np.int64)).to(d)
    gT = torch.as_tensor(np.ascontiguousarray(np.asarray(T0, np.float64)[:, :3])).to(d)
    T = torch.full((P, 12), sentinel, dtype=torch.float64, device=d)
    fit, rm = (torch.full((P,), sentinel, dtype=torch.float64, device=d) for _ in range(2))
    nc, it, st = (torch.full((P,), int(sentinel), dtype=torch.int32, device=d) for _ in range(3))
    tr = torch.full((P, max_iters + 1, 2), sentinel, dtype=torch.float64, device=d)
    N.check(N.lib().mvr_icp_refine(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.off_dev), fo.B, fo.M,
                                   fo.r, N.ptr(gp), N.ptr(gT), P, max_dist, max_iters, tol, tol, N.ptr(T), N.ptr(fit),
                                   N.ptr(rm), N.ptr(nc), N.ptr(it), N.ptr(st), N.ptr(tr), N.stream()),
            "mvr_icp_refine")
    T4 = np.tile(np.eye(4), (P, 1, 1))
    T4[:, :3] = T.cpu().numpy().reshape(P, 3, 4)
    return {"T": T4, "fitness": fit.cpu().numpy(), "rmse": rm.cpu().numpy(), "n_corr": nc.cpu().numpy(),
            "iters": it.cpu().numpy(), "status": st.cpu().numpy(), "trace": tr.cpu().numpy()}


def test_small_shapes_and_invalid_pairs_in_one_batch(gpu):
    from lib.overlap import FragmentOverlap
    frags, pairs, T0 = O.small_case()
    fo = FragmentOverlap(frags, "3DMatch", radius=O.SMALL_RADIUS)
    assert fo.r == O.SMALL_RADIUS and fo.B == len(frags)
    cells = frags[0] / O.SMALL_RADIUS
    assert (frags[0].min(0) < -0.3).all() and np.any(np.abs(cells - np.round(cells)) < 1e-12)   # on cell faces
    # two invalid pairs among the others: a NaN in T0 (with a payload), a fragment index B
    T_nan = T0[4].copy()
    T_nan[1, 2] = np.frombuffer(np.uint64(0x7FF8000000ABCDEF).tobytes(), np.float64)[0]
    pairs = np.concatenate([pairs[:3], [[4, 0]], pairs[3:6], [[len(frags), 0]], pairs[6:]])
    T0 = np.concatenate([T0[:3], T_nan[None], T0[3:6], T0[5:6], T0[6:]])
    want = O.icp_batch(frags, pairs, T0, O.SMALL_MAX_DIST, 30, 0.0, 0.0)
    got = _raw_call(fo, pairs, T0, O.SMALL_MAX_DIST, 30, 0.0)
    assert [w["status"] for w in want] == [1, 1, 1, 4, 0, 0, 0, 4, 0, 0, 1]
    for name in ("T", "fitness", "rmse", "n_corr", "iters", "status", "trace"):
        assert not np.any(got[name] == -77.0), name                     # every row of every output is written
    _compare(got, want)
    for k in (0, 1, 2, 10):      # 0, 1, 2 source points, and the start that leaves no correspondence: T = T0
        np.testing.assert_array_equal(got["T"][k][:3], T0[k][:3])
        assert got["iters"][k] == 0 and (got["trace"][k][1:] == -1.0).all()
    assert got["fitness"][0] == 0.0 and got["fitness"][1] == 1.0 and got["fitness"][2] == 1.0
    for k in (3, 7):             # invalid: T0 copied bit for bit, everything else 0, no evaluation in the trace
        assert got["T"][k][:3].tobytes() == np.ascontiguousarray(T0[k][:3]).tobytes()
        assert (got["fitness"][k], got["rmse"][k], got["n_corr"][k], got["iters"][k]) == (0.0, 0.0, 0, 0)
        assert (got["trace"][k] == -1.0).all()
    # the neighbours of the invalid pairs are what they are without them
    ok = [k for k in range(len(pairs)) if k not in (3, 7)]
    alone = _raw_call(fo, pairs[ok], T0[ok], O.SMALL_MAX_DIST, 30, 0.0)
    for name in alone:
        assert alone[name].tobytes() == got[name][ok].tobytes(), name


# --------------------------------------------------------------------------------------------------- batch invariance
def test_outputs_do_not_depend_on_the_batch(gpu):
    from lib.icp import icp_refine
    fo = _fo("FCGF")
    T6 = _six_starts()
    ref, _ = _six(0.075, 30, 0.0)

    def same(got, rows, where):
        for name in ref:
            assert np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(ref[name][rows]).tobytes(), \
                (where, name)

    for k in range(6):                                                  # each pair alone
        same(icp_refine(fo, [O.SIX[k]], T6[k:k + 1], 0.075, 30, 0.0, 0.0, return_trace=True), [k], "alone %d" % k)
    perm = np.random.default_rng(1).permutation(6)                      # shuffled
    same(icp_refine(fo, np.asarray(O.SIX)[perm], T6[perm], 0.075, 30, 0.0, 0.0, return_trace=True), perm, "shuffled")
    rows = np.array([0, 1, 2, 0, 1, 0, 5, 2, 2, 0, 0])                  # fragment 0 the source of several pairs
    same(icp_refine(fo, np.asarray(O.SIX)[rows], T6[rows], 0.075, 30, 0.0, 0.0, return_trace=True), rows, "repeated")


# ----------------------------------------------------------------------------------------------------- Python surface
def test_python_surface_dtypes_and_devices(gpu):
    import torch
    from lib.icp import icp_refine, icp_pair
    fo = _fo("FCGF")
    T6 = _six_starts()
    ref, _ = _six(0.075, 30, 1e-6)
    # fp64 torch on the device in -> torch on the device out, the same bits
    dev_out = icp_refine(fo, torch.tensor(O.SIX, device=gpu), torch.from_numpy(T6).to(gpu), 0.075, return_trace=True)
    assert all(torch.is_tensor(v) and v.device.type == "cuda" for v in dev_out.values())
    assert dev_out["T"].shape == (6, 4, 4) and dev_out["trace"].shape == (6, 31, 2)
    assert dev_out["n_corr"].dtype == torch.int32 and dev_out["T"].dtype == torch.float64
    for name in ref:
        assert dev_out[name].cpu().numpy().tobytes() == ref[name].tobytes(), name
    # [P,3,4] and fp32 inputs (torch on the host -> torch on the host, numpy -> numpy): the fp32 start, in fp64
    T32 = T6[:, :3].astype(np.float32)
    want = icp_refine(fo, O.SIX, T32.astype(np.float64), 0.075)
    for Tin in (torch.from_numpy(T32), T32):
        out = icp_refine(fo, O.SIX, Tin, 0.075)
        assert all((torch.is_tensor(v) and v.device.type == "cpu") if torch.is_tensor(Tin) else
                   isinstance(v, np.ndarray) for v in out.values()) and "trace" not in out
        for name in want:
            assert np.asarray(out[name]).tobytes() == want[name].tobytes(), name
    # icp_pair: raw points = icp_refine on a two-fragment raw index; voxel_size = on the centroids
    frags = O.scene4()[0]
    src, tgt, T_one, max_dist, iters = O.pair_case()
    one = icp_pair(src, tgt, T_one, max_dist=max_dist, max_iters=iters)
    w = O.icp(src, tgt, T_one, max_dist, iters)
    assert one["T"].shape == (4, 4) and int(one["n_corr"]) == w["n_corr"] and int(one["iters"]) == w["iters"]
    assert np.abs(one["T"][:3] - w["T"]).max() <= TOL and abs(one["rmse"] - w["rmse"]) <= TOL
    vox = icp_pair(torch.from_numpy(frags[0]), torch.from_numpy(frags[1]), torch.from_numpy(T6[0]), max_dist=0.075,
                   voxel_size=0.025, max_iters=30, tol_fitness=0.0, tol_rmse=0.0, return_trace=True)
    full, _ = _six(0.075, 30, 0.0)
    assert torch.is_tensor(vox["T"]) and int(vox["n_corr"]) == int(full["n_corr"][0])
    np.testing.assert_allclose(vox["T"].numpy(), full["T"][0], rtol=0, atol=TOL)      # the two-fragment index
    np.testing.assert_allclose(vox["trace"].numpy(), full["trace"][0], rtol=0, atol=TOL)


# ------------------------------------------------------------------------------------------------------------ harness
def test_benchmark_harness_with_icp(gpu, tmp_path):
    """--icp refines every pair's estimate on the batch's FragmentOverlap before the inversion: every written
    transform equals inv(icp_refine(.)) of the run without the flag; the flag's absence changes nothing."""
    import shutil
    from eval_layout import write_scene, read_results
    from lib.icp import icp_refine
    from lib.overlap import FragmentOverlap
    from lib.utils import read_trajectory
    from scripts.benchmark_pairwise_registration import main
    roots = [str(tmp_path / n) for n in ("plain", "icp", "plain2")]
    pairs = write_scene(os.path.join(roots[0], "3d_match"), "kitchen", 4, 600, seed=0)
    for r in roots[1:]:
        shutil.copytree(roots[0], r)
    argv = ["--method", "RANSAC", "--batch_size", "4", "--num_workers", "0"]
    s0 = main(["--source_path", roots[0]] + argv)
    s1 = main(["--source_path", roots[1]] + argv + ["--icp", "--icp_iters", "20"])
    s2 = main(["--source_path", roots[2]] + argv)
    assert read_results(roots[0], "3d_match", "RANSAC") == read_results(roots[2], "3d_match", "RANSAC")
    assert s0 == s2 and s1["recall"] == 1.0 and s1["precision"] == 1.0
    traj = []
    for r in roots[:2]:
        keys, t = read_trajectory(os.path.join(r, "3d_match", "results", "RANSAC", "all", "kitchen", "traj.txt"))
        assert keys.tolist() == [[str(i), str(j), "True"] for i, j in pairs] and t.shape == (6, 4, 4)
        traj.append(t)
    clouds = [np.load(os.path.join(roots[0], "3d_match", "features", "kitchen", "kitchen_%03d.npz" % k))["xyz"]
              for k in range(4)]
    fo = FragmentOverlap(clouds, "FCGF")
    ref = icp_refine(fo, pairs, np.linalg.inv(traj[0]), max_iters=20)
    print("refined vs plain: %.3g; written vs inv(icp_refine): %.3g"
          % (np.abs(traj[1] - traj[0]).max(), np.abs(traj[1] - np.linalg.inv(ref["T"])).max()))
    # the files hold 12 decimals and the refinement restarts from them: the scene's fragments are exact copies, so
    # one solve lands on the same fixed point from either start
    np.testing.assert_allclose(traj[1], np.linalg.inv(ref["T"]), rtol=0, atol=1e-9)
    assert not np.array_equal(traj[1], traj[0])
