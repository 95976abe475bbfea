"""GPU Fast Global Registration (csrc/fgr.hip mvr_fgr, lib.utils.run_fgr_batch, lib.fpfh.register_fgr,
lib.multiview.register_scene(coarse="fgr"), the two CLIs) against the numpy restatement (tests/fgr_oracle.py).

Tolerances.  The tuple filter's comparisons are rounded fp64 operations on both sides and tests/test_fgr_host.py keeps
every one of them 2.8e-7 or more (relative) from equality: n_tuples, n_used and status are compared exactly.  T,
fitness, rmse and the trace differ from the oracle by the order of the sums only; the project's fp64 bound of 1e-9
holds them, and the host test measures 1.3e-15 for a perturbation of the last bits: orders of margin.  fitness is an
inlier count over n: no final distance lies within 1e-7 of max_dist (host test), so it is exact up to its division."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import fgr_oracle as F
import icp_oracle as O

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
DEMO = os.path.join(GOLDEN, "demo")
DEMO_CFG = os.path.join(GOLDEN, "configs", "pairwise_registration", "demo", "config.yaml")
KEYS = ("T", "fitness", "rmse", "n_used", "n_tuples", "status", "trace")


def _raw(x1, x2, counts, tuple_test=True, seed=F.SEED, **over):
    """mvr_fgr on sentinel-filled output buffers -> run_fgr_batch's dict with the trace"""
    import torch
    from lib import _native as N
    o = dict(F.DEFAULTS, **over)
    dev = torch.device("cuda:0")
    a = torch.from_numpy(np.array(x1, dtype=np.float64)).to(dev)      # a copy: the shared batch is read-only
    b = torch.from_numpy(np.array(x2, dtype=np.float64)).to(dev)
    P, n = a.shape[0], a.shape[1]
    cnt = torch.as_tensor(np.asarray(counts, np.int32)).to(dev)
    T = torch.full((P, 4, 4), SENTINEL, dtype=torch.float64, device=dev)
    fit, rmse = (torch.full((P,), SENTINEL, dtype=torch.float64, device=dev) for _ in range(2))
    n_used, n_tuples, status = (torch.full((P,), -77, dtype=torch.int32, device=dev) for _ in range(3))
    trace = torch.full((P, o["iters"], 2), SENTINEL, dtype=torch.float64, device=dev)
    L = N.lib()
    ws = torch.full((L.mvr_fgr_workspace_bytes(P, n, o["max_tuples"]),), 0x7F, dtype=torch.uint8, device=dev)
    N.check(L.mvr_fgr(N.ptr(a), N.ptr(b), 3 * n, N.ptr(cnt), P, o["max_dist"], o["iters"], o["division_factor"],
                      o["tuple_factor"] if tuple_test else 0, o["max_tuples"], o["tuple_scale"], seed, N.ptr(T),
                      N.ptr(fit), N.ptr(rmse), N.ptr(n_used), N.ptr(n_tuples), N.ptr(status), N.ptr(trace), N.ptr(ws),
                      ws.numel(), N.stream()), "mvr_fgr")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(KEYS, (T, fit, rmse, n_used, n_tuples, status, trace))}


def _same_bytes(a, b, keys=KEYS):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def _close(got, want, rows=None):
    """got (arrays over pairs) against want (F.stacked): the integers exactly, the rest within 1e-9"""
    rows = slice(None) if rows is None else rows
    for k in ("n_tuples", "n_used", "status"):
        assert got[k][rows].tolist() == want[k][rows].tolist(), k
    for k in ("T", "fitness", "rmse", "trace"):
        d = np.abs(got[k][rows] - want[k][rows])
        print("%s: largest difference from the oracle %.3g" % (k, d.max() if d.size else 0.0))
        np.testing.assert_allclose(got[k][rows], want[k][rows], rtol=0, atol=1e-9, err_msg=k)


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("tuple_test", [True, False])
def test_batch_matches_the_oracle(gpu, tuple_test):
    from lib.utils import run_fgr_batch
    x1, x2, counts = F.batch()
    got = _raw(x1, x2, counts, tuple_test)
    for k in KEYS:
        assert np.isfinite(got[k]).all() and not (got[k] == SENTINEL).any(), k
    _close(got, F.stacked(F.batch_results(tuple_test)))
    assert got["status"][:3].tolist() == [1, 1, 1] and (got["status"][3:] == 0).all()
    np.testing.assert_array_equal(got["T"][:3], np.tile(np.eye(4), (3, 1, 1)))
    assert not got["fitness"][:3].any() and not got["rmse"][:3].any() and (got["trace"][:3] == -1.0).all()
    assert (got["T"][:, 3] == [0.0, 0.0, 0.0, 1.0]).all()
    np.testing.assert_allclose(np.linalg.det(got["T"][:, :3, :3]), 1.0, rtol=0, atol=1e-9)
    # the Python surface: the same bytes, with and without the trace
    y1, y2 = np.array(x1), np.array(x2)                # copies: the shared batch is read-only
    api = run_fgr_batch(y1, y2, counts, seed=F.SEED, max_dist=F.MAX_DIST, tuple_test=tuple_test, return_trace=True)
    assert set(api) == set(KEYS) and _same_bytes(api, got)
    plain = run_fgr_batch(y1, y2, counts, seed=F.SEED, max_dist=F.MAX_DIST, tuple_test=tuple_test)
    assert set(plain) == set(KEYS) - {"trace"} and _same_bytes(plain, got, [k for k in KEYS if k != "trace"])


def test_two_runs_and_a_pair_alone_give_the_same_bytes(gpu):
    x1, x2, counts = F.batch()
    for tuple_test in (True, False):
        a, b = _raw(x1, x2, counts, tuple_test), _raw(x1, x2, counts, tuple_test)
        assert _same_bytes(a, b)
        for p in (4, 10, 11):      # alone at the same p (the draws are keyed by p): the pairs before it empty
            alone = _raw(x1[:p + 1], x2[:p + 1], [0] * p + [int(counts[p])], tuple_test)
            assert all(alone[k][p].tobytes() == a[k][p].tobytes() for k in KEYS), (tuple_test, p)
            assert (alone["status"][:p] == 1).all()


def test_a_shift_of_both_clouds_moves_the_translation_only(gpu):
    """x -> x + s in both clouds: R stays and t' = t + s - R s, both within the project's fp64 bound of 1e-9.  The
    shifted coordinates are rounded at magnitude |s| = 229 (2.8e-14 absolute on clouds of size 3, 1e-14 relative),
    the host test measures an amplification near 1 for such perturbations, and R's change acts on t' with the lever
    |s|: about 229 x 1e-14 = 2e-12 is expected, orders below the bound (measured: the oracle on the shifted clouds
    1.7e-13, the GPU 2.3e-13 on t and 6.7e-16 on R)."""
    x1, x2, counts = F.batch()
    s = np.array([100.0, -200.0, 50.0])
    for tuple_test in (True, False):
        a = _raw(x1, x2, counts, tuple_test)
        b = _raw(x1 + s, x2 + s, counts, tuple_test)
        for p in (9, 10):
            assert b["n_tuples"][p] == a["n_tuples"][p] and b["status"][p] == 0
            R, t = a["T"][p, :3, :3], a["T"][p, :3, 3]
            print("shift, tuple filter %s, case %d: |dR| %.3g, |dt| %.3g"
                  % (tuple_test, p, np.abs(b["T"][p, :3, :3] - R).max(),
                     np.abs(b["T"][p, :3, 3] - (t + s - R @ s)).max()))
            np.testing.assert_allclose(b["T"][p, :3, :3], R, rtol=0, atol=1e-9)
            np.testing.assert_allclose(b["T"][p, :3, 3], t + s - R @ s, rtol=0, atol=1e-9)
            assert abs(b["fitness"][p] - a["fitness"][p]) < 1e-9 and abs(b["rmse"][p] - a["rmse"][p]) < 1e-9


# ---------------------------------------------------------------------------------------------------------- settings
def test_settings(gpu):
    x1, x2, counts = F.batch()

    def one(p, tuple_test=True, **over):
        got = _raw(x1, x2, counts, tuple_test, **over)
        want = F.fgr(x1[p, :counts[p]], x2[p, :counts[p]], seed=F.SEED, p=p, tuple_test=tuple_test,
                     **dict(F.DEFAULTS, **over))
        _close({k: got[k][p:p + 1] for k in KEYS}, F.stacked([want]))
        return got, want

    # iters = 0: the start of the loop (R = I, t = 0 between the centred clouds) and its evaluation
    got, want = one(10, iters=0)
    assert got["trace"].shape == (len(counts), 0, 2)
    np.testing.assert_array_equal(got["T"][10, :3, :3], np.eye(3))
    n = counts[10]
    np.testing.assert_allclose(got["T"][10, :3, 3], x2[10, :n].mean(0) - x1[10, :n].mean(0), rtol=0, atol=1e-12)
    assert got["n_tuples"][10] == 1000 and got["status"][10] == 0 and got["fitness"][10] == want["fitness"]
    # max_tuples = 7: the first 7 passing tests of case 10
    got, want = one(10, max_tuples=7)
    assert got["n_tuples"][10] == 7 and got["n_used"][10] == 21 == want["n_used"]
    # tuple_factor = 1 on case 11 (2000 tests at 5 % inliers): few or no tuples, handled by status
    got, want = one(11, tuple_factor=1)
    assert got["n_tuples"][11] == want["n_tuples"] == 1 and got["n_used"][11] == 3 and got["status"][11] == 0
    got, want = one(11, tuple_factor=1, tuple_scale=1.0)      # no noisy tuple has three equal edge pairs
    assert got["n_tuples"][11] == 0 and got["status"][11] == 1 and not got["T"][11, :3, 3].any()
    # another seed, division factor and scale on a case below the cap
    got, want = one(9, division_factor=2.0, tuple_scale=0.9, iters=30)
    assert got["trace"][9, 0, 0] == 0.5
    x = _raw(x1, x2, counts, seed=12345)
    want = F.fgr(x1[9, :300], x2[9, :300], seed=12345, p=9)
    assert x["n_tuples"][9] == want["n_tuples"] == 893 and F.batch_results(True)[9]["n_tuples"] == 842
    np.testing.assert_allclose(x["T"][9], want["T"], rtol=0, atol=1e-9)


def test_status_paths(gpu):
    """bit 8 (three collinear correspondences: T is the loop's last, here its start), bit 4 (a non-finite row, also
    one beyond the used rows' reach of the tuple filter), bit 1 (coincident points: scale 0)"""
    n = 6
    x1 = np.zeros((4, n, 3))
    x2 = np.zeros((4, n, 3))
    line = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]])
    x1[0, :3], x2[0, :3] = line, line + [0.5, 0.25, -1.0]
    rng = np.random.default_rng(3)
    x1[1] = rng.uniform(-1, 1, (n, 3))
    x2[1] = x1[1] + 0.1
    x2[1, 5, 1] = np.inf
    x1[2], x2[2] = 1.0, 2.0
    x1[3] = x1[1]
    x2[3] = x1[1] + 0.1
    x1[3, 5, 0] = np.nan                       # beyond counts: not looked at
    counts = [3, 6, 5, 5]
    for tuple_test in (False, True):
        got = _raw(x1, x2, counts, tuple_test)
        want = [F.fgr(x1[p, :c], x2[p, :c], p=p, tuple_test=tuple_test) for p, c in enumerate(counts)]
        assert [w["status"] for w in want] == [8, 4, 1, 0]
        _close(got, F.stacked(want))
        for p in (1, 2):
            np.testing.assert_array_equal(got["T"][p], np.eye(4))
            assert got["fitness"][p] == 0.0 and got["rmse"][p] == 0.0 and (got["trace"][p] == -1.0).all()
        np.testing.assert_array_equal(got["T"][0, :3, :3], np.eye(3))
        np.testing.assert_allclose(got["T"][0, :3, 3], [0.5, 0.25, -1.0], rtol=0, atol=1e-12)
        assert got["fitness"][0] == 1.0 and got["trace"][0, 0, 0] == 1.0 / 1.4 and (got["trace"][0, 1:] == -1.0).all()
        np.testing.assert_allclose(got["T"][3, :3, 3], [0.1, 0.1, 0.1], rtol=0, atol=1e-9)


# -------------------------------------------------------------------------------------------------------- end to end
def _rot_deg(Ra, Rb):
    return np.rad2deg(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def test_register_fgr_recovers_a_full_copy_and_feeds_icp(gpu):
    """the fixture of test_gpu_fpfh.py's RANSAC test (icp_oracle.full_copy_case on fragment 0's centroids, normals
    towards the moved viewpoint, FPFH over 0.075).  The CPU chain (oracle normals and FPFH, mutual matches, the numpy
    FGR) found 1277 mutual matches, 1127 of them true, and ended 0.0002 m and 0.02 degrees off in both modes."""
    from lib.fpfh import correspondences, match_features, register_fgr
    from lib.icp import icp_refine
    from lib.overlap import FragmentOverlap
    from lib.utils import RANSAC_DIST, run_fgr_batch
    src = O.scene4_centroids()[0]
    tgt, Tt, _ = O.full_copy_case(src)
    c = src.mean(0)
    fo = FragmentOverlap([src, tgt], "3DMatch", radius=0.075)
    fo.estimate_normals(viewpoints=np.asarray([c, Tt[:3, :3] @ c + Tt[:3, 3]]))
    fo.compute_fpfh(0.075)
    matches = match_features(fo.fpfh, fo.off, [[0, 1]])
    xs, xt = correspondences(fo, [[0, 1]], matches)
    for tuple_test in (True, False):
        out = register_fgr(fo, [[0, 1]], seed=0, tuple_test=tuple_test)
        T = out["T"][0]
        dt = np.linalg.norm((T[:3, :3] @ c + T[:3, 3]) - (Tt[:3, :3] @ c + Tt[:3, 3]))
        dr = _rot_deg(T[:3, :3], Tt[:3, :3])
        print("register_fgr(tuple_test=%s): %d mutual matches, %d tuples, fitness %.3f, rmse %.4f; off by %.4f m at "
              "the centroid, %.3f deg" % (tuple_test, out["n_matches"][0], out["n_tuples"][0], out["fitness"][0],
                                          out["rmse"][0], dt, dr))
        assert set(out) == {"T", "fitness", "rmse", "n_matches", "n_used", "n_tuples", "status"}
        assert out["T"].shape == (1, 4, 4) and out["status"][0] == 0 and out["n_matches"][0] == len(matches[0])
        assert dt <= RANSAC_DIST and dr <= 1.0
        by_hand = run_fgr_batch(xs, xt, [len(matches[0])], seed=0, tuple_test=tuple_test)
        assert all(by_hand[k].tobytes() == out[k].tobytes() for k in by_hand)
        ref = icp_refine(fo, [[0, 1]], out["T"], max_dist=0.05, max_iters=30, tol_fitness=0.0, tol_rmse=0.0)
        print("icp_refine from it: |T - T_true| %.3g, rmse %.3g" % (np.abs(ref["T"][0] - Tt).max(), ref["rmse"][0]))
        np.testing.assert_allclose(ref["T"][0], Tt, rtol=0, atol=1e-9)
    with pytest.raises(ValueError):
        register_fgr(fo, [[0, 1]], counts=[3])


def test_register_fgr_without_matches(gpu):
    """pairs with an empty fragment: no match, the identity, status 1"""
    import torch
    import fpfh_oracle as FO
    from lib.fpfh import register_fgr
    from lib.overlap import FragmentOverlap
    frags, normals = FO.small_case()                   # test_gpu_fpfh.py's construction: sizes 0, 1, 2, 3, 63
    fo = FragmentOverlap(frags[:5], "3DMatch", radius=FO.SMALL_R_INDEX)
    fo.normals = torch.from_numpy(np.concatenate(normals[:5]).reshape(-1, 3)).to(fo.device).contiguous()
    fo.compute_fpfh()
    out = register_fgr(fo, [[0, 4], [4, 0], [4, 4]])
    assert out["n_matches"].tolist() == [0, 0, 63] and out["status"].tolist() == [1, 1, 0]
    np.testing.assert_array_equal(out["T"][:2], np.tile(np.eye(4), (2, 1, 1)))
    np.testing.assert_allclose(out["T"][2], np.eye(4), rtol=0, atol=1e-9)       # a fragment onto itself
    assert out["n_used"][:2].tolist() == [0, 0] and out["n_used"][2] == 3 * out["n_tuples"][2] > 0
    none = register_fgr(fo, np.zeros((0, 2), np.int64))
    assert none["T"].shape == (0, 4, 4) and set(none) == set(out)


def test_register_scene_coarse_fgr_is_register_fgr(gpu):
    """plumbing, not quality (the scene's FPFH matches hold a few percent inliers, FGR's field is
    tens of percent): T_coarse is register_fgr's output on the returned fo, keys and shapes as with RANSAC.  The
    gate at 0 keeps every pair in both runs."""
    from lib.fpfh import register_fgr
    from lib.multiview import register_scene
    raw = O.scene4()[0]
    res = register_scene(raw, 0.025, seed=3, overlap_threshold=0.0, coarse="fgr")
    base = register_scene(raw, 0.025, seed=3, overlap_threshold=0.0)
    rec = res["pairs"]
    want = register_fgr(res["fo"], rec["pairs"], seed=3)
    assert rec["T_coarse"].tobytes() == want["T"].tobytes() and rec["pairs"].tolist() == [list(p) for p in O.SIX]
    assert rec["T_coarse"].tobytes() != base["pairs"]["T_coarse"].tobytes()
    print("FGR on the scene's FPFH matches: matches %s, tuples %s, status %s, fitness %s"
          % (want["n_matches"], want["n_tuples"], want["status"], np.round(want["fitness"], 3)))
    assert set(res) == set(base) and set(rec) == set(base["pairs"])
    for k in rec:
        assert rec[k].shape == base["pairs"][k].shape and rec[k].dtype == base["pairs"][k].dtype, k
    for k in ("R", "t", "poses", "member"):
        assert np.asarray(res[k]).shape == np.asarray(base[k]).shape, k
    with pytest.raises(ValueError):
        register_scene(raw, 0.025, coarse="fgr", ransac_checkers=True)


# --------------------------------------------------------------------------------------------------------------- CLI
def test_register_scene_cli_coarse_fgr(gpu, tmp_path, capsys):
    from lib.ply import write_ply_xyz
    from scripts.fuse_scene import read_poses
    from scripts.register_scene import main
    files = []
    for b, f in enumerate(O.scene4()[0]):
        files.append(str(tmp_path / ("frag_%d.ply" % b)))
        write_ply_xyz(files[-1], f[::2])
    out = str(tmp_path / "out")
    res = main(["--fragments"] + files + ["--out", out, "--coarse", "fgr", "--seed", "1"])
    assert "registered 4 fragments" in capsys.readouterr().out
    np.testing.assert_allclose(read_poses(out + "/poses.txt", 4), res["poses"], rtol=0, atol=1e-11)
    assert os.path.exists(out + "/traj.txt") and os.path.exists(out + "/scene.ply")
    with pytest.raises(SystemExit):
        main(["--fragments"] + files + ["--out", out, "--coarse", "fgr", "--checkers"])


def test_pairwise_demo_fgr(gpu, tmp_path, monkeypatch, capsys):
    """scripts/pairwise_demo.py --fpfh --fgr on the demo pair: no checkpoint; the pair has no ground truth here, its
    fitness is printed, not asserted"""
    from lib.utils import load_config, read_trajectory
    from scripts.pairwise_demo import main, parser
    src, tgt = os.path.join(DEMO, "cloud_bin_0.ply"), os.path.join(DEMO, "cloud_bin_1.ply")
    monkeypatch.chdir(tmp_path)
    a = parser().parse_args([DEMO_CFG, "--source_pc", src, "--target_pc", tgt, "--fpfh", "--fgr"])
    T = main(load_config(a.config), a)
    printed = capsys.readouterr().out
    print(printed)
    assert "FGR: fitness" in printed and "T (source -> target)" in printed
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-9 and (T[3] == [0.0, 0.0, 0.0, 1.0]).all()
    _, traj = read_trajectory(str(tmp_path / "data/demo/pairwise/results/est_T.log"))
    np.testing.assert_allclose(traj[0], T, atol=1e-9)
    for bad in (["--fgr"], ["--fpfh", "--fgr", "--checkers"]):
        b = parser().parse_args([DEMO_CFG, "--source_pc", src, "--target_pc", tgt] + bad)
        with pytest.raises(ValueError):
            main(load_config(b.config), b)
