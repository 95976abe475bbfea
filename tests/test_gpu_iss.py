"""GPU ISS keypoints (csrc/iss.hip mvr_iss_saliency / mvr_radius_nms, lib.overlap.FragmentOverlap.iss_keypoints) and
the matching on keypoints built on them (lib.fpfh.match_keypoints, register_fpfh / register_fgr /
register_scene(keypoints=...), the two scripts) against the numpy oracle (tests/iss_oracle.py).

Tolerances.  n_nbr, the candidate set and the -1.0 of every other point must equal the oracle's exactly: every
distance is at least 1e-7 (relative) from its radius and every eigenvalue ratio at least 1e-6 from its threshold
(tests/test_iss_host.py asserts both on these cases), far above the 1e-13 two fp64 evaluations differ by.  A
candidate's saliency l3 is within 1e-9 l1 of the oracle's, the project's fp64 bound (the normals'); the largest error
is printed.  mvr_radius_nms is a pure function of comparisons, so on any given score array it must equal the oracle's
NMS of that array exactly, no point left out.  End to end against the pure oracle, keep is compared where the
deciding score is at least 1e-9 (relative) away; the share left out is capped at 2 % of the candidates."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
import icp_oracle as O
import iss_oracle as I
import knn_oracle as K

pytestmark = pytest.mark.gpu
GUARD = 3
S_SAL, S_N, S_KEEP = -77.0, -77, 77
DEMO = os.path.join(GOLDEN, "demo")
DEMO_CFG = os.path.join(GOLDEN, "configs", "pairwise_registration", "demo", "config.yaml")


def _index(dev, frags, r):
    import torch
    from lib import _native as N
    L = N.lib()
    off = K.offsets(frags)
    M = int(off[-1])
    xyz = torch.from_numpy(K.stack(frags)).to(dev)
    g_off = torch.from_numpy(off).to(dev)
    ib = L.mvr_radius_index_bytes(M)
    index = torch.empty(ib, dtype=torch.uint8, device=dev)
    assert L.mvr_radius_index_build(N.ptr(xyz), N.ptr(g_off), len(frags), M, r, N.ptr(index), ib, N.stream()) == 0
    return {"index": index, "ib": ib, "xyz": xyz, "off": g_off, "B": len(frags), "M": M, "r": r}


def _raw_saliency(ix, radius, g21=I.GAMMA_21, g32=I.GAMMA_32, min_ratio=I.MIN_RATIO, min_n=I.MIN_NEIGHBORS):
    """mvr_iss_saliency through the C ABI on sentinel-filled outputs with guard rows -> (saliency, n_nbr) numpy;
    every row written, nothing behind them"""
    import torch
    from lib import _native as N
    M, dev = ix["M"], ix["xyz"].device
    sal = torch.full((M + GUARD,), S_SAL, dtype=torch.float64, device=dev)
    n_nbr = torch.full((M + GUARD,), S_N, dtype=torch.int32, device=dev)
    assert N.lib().mvr_iss_saliency(N.ptr(ix["index"]), ix["ib"], N.ptr(ix["xyz"]), N.ptr(ix["off"]), ix["B"], M,
                                    ix["r"], radius, g21, g32, min_ratio, min_n, N.ptr(sal), N.ptr(n_nbr),
                                    N.stream()) == 0
    assert (sal[M:] == S_SAL).all() and (n_nbr[M:] == S_N).all()
    sal, n_nbr = sal[:M].cpu().numpy(), n_nbr[:M].cpu().numpy()
    assert not (sal == S_SAL).any() and not (n_nbr == S_N).any()
    return sal, n_nbr


def _raw_nms(ix, radius, score, min_n=I.MIN_NEIGHBORS):
    """mvr_radius_nms on a sentinel-filled keep with guard rows -> bool numpy; every row written as 0 or 1"""
    import torch
    from lib import _native as N
    M, dev = ix["M"], ix["xyz"].device
    g_score = torch.from_numpy(np.ascontiguousarray(score, dtype=np.float64)).to(dev)
    keep = torch.full((M + GUARD,), S_KEEP, dtype=torch.uint8, device=dev)
    assert N.lib().mvr_radius_nms(N.ptr(ix["index"]), ix["ib"], N.ptr(ix["xyz"]), N.ptr(ix["off"]), ix["B"], M,
                                  ix["r"], radius, min_n, N.ptr(g_score), N.ptr(keep), N.stream()) == 0
    assert (keep[M:] == S_KEEP).all()
    keep = keep[:M].cpu().numpy()
    assert np.isin(keep, (0, 1)).all()
    return keep.astype(bool)


def _same_saliency(what, sal, n_nbr, want):
    """(a): n_nbr and the candidate set exact, -1.0 exact, l3 within 1e-9 l1"""
    np.testing.assert_array_equal(n_nbr, want["n_nbr"], err_msg=what)
    cand = sal != -1.0
    np.testing.assert_array_equal(cand, want["candidate"], err_msg=what)
    err = np.abs(sal[cand] - want["saliency"][cand]) / want["eig"][cand, 0]
    print("%s: %d points, %d candidates; largest |l3 - oracle| / l1 = %.3g" % (what, len(sal), cand.sum(),
                                                                               err.max() if cand.any() else 0.0))
    assert (err <= 1e-9).all() and (sal[cand] > 0).all()


# ------------------------------------------------------------------------------------------- (a), (b), (c): the ABI
@pytest.mark.parametrize("name", I.CASES)
def test_saliency_and_nms_match_the_oracle(gpu, name):
    frags, r_index, sal_r, nms_r = I.case(name)
    want_s, want_n = I.case_oracle(name)
    pts, off = K.stack(frags), K.offsets(frags)
    ix = _index(gpu, frags, r_index)
    sal, n_nbr = _raw_saliency(ix, sal_r)
    _same_saliency(name, sal, n_nbr, want_s)                                     # (a)
    if name != "clouds":
        assert (sal[:off[4]] == -1.0).all() and (sal[off[I.PLANAR]:off[I.PLANAR + 1]] == -1.0).all()
    keep = _raw_nms(ix, nms_r, sal)
    own = I.nms(pts, off, nms_r, I.MIN_NEIGHBORS, sal)                           # (b): the GPU's own saliency
    np.testing.assert_array_equal(keep, own["keep"])
    robust = want_n["margin"] >= 1e-9                                            # (c): the pure oracle
    left_out = int((~robust).sum())
    print("%s: %d keypoints; %d of %d candidates left out of the end-to-end comparison"
          % (name, keep.sum(), left_out, want_s["candidate"].sum()))
    assert left_out <= 0.02 * want_s["candidate"].sum()
    np.testing.assert_array_equal(keep[robust], want_n["keep"][robust])
    again_s, again_n = _raw_saliency(ix, sal_r)
    assert again_s.tobytes() == sal.tobytes() and again_n.tobytes() == n_nbr.tobytes()
    assert _raw_nms(ix, nms_r, again_s).tobytes() == keep.tobytes()
    # n_nbr may be NULL
    import torch
    from lib import _native as N
    only = torch.empty(ix["M"], dtype=torch.float64, device=gpu)
    assert N.lib().mvr_iss_saliency(N.ptr(ix["index"]), ix["ib"], N.ptr(ix["xyz"]), N.ptr(ix["off"]), ix["B"],
                                    ix["M"], ix["r"], sal_r, I.GAMMA_21, I.GAMMA_32, I.MIN_RATIO, I.MIN_NEIGHBORS,
                                    N.ptr(only), None, N.stream()) == 0
    assert only.cpu().numpy().tobytes() == sal.tobytes()


def test_fragments_in_the_same_space_give_the_bits_each_gives_alone(gpu):
    frags, r_index, sal_r, nms_r = I.case("small")
    off = K.offsets(frags)
    ix = _index(gpu, frags, r_index)
    sal, n_nbr = _raw_saliency(ix, sal_r)
    keep = _raw_nms(ix, nms_r, sal)
    for b in (3, 4, 6, 7):
        one = _index(gpu, [frags[b]], r_index)
        s1, n1 = _raw_saliency(one, sal_r)
        rows = slice(off[b], off[b + 1])
        assert s1.tobytes() == sal[rows].tobytes() and n1.tobytes() == n_nbr[rows].tobytes(), b
        assert _raw_nms(one, nms_r, s1).tobytes() == keep[rows].tobytes(), b


def test_other_thresholds_and_open3ds_rule(gpu):
    """gammas, min_neighbors and min_ratio reach the kernel: looser gammas and min_ratio 0 against the oracle's n_nbr
    and, where the margins hold, its candidates"""
    frags, r_index, sal_r, _ = I.case("small_075")
    pts, off = K.stack(frags), K.offsets(frags)
    ix = _index(gpu, frags, r_index)
    want = I.saliency(pts, off, sal_r, 0.8, 0.6, 1e-3, 12)
    sal, n_nbr = _raw_saliency(ix, sal_r, 0.8, 0.6, 1e-3, 12)
    np.testing.assert_array_equal(n_nbr, want["n_nbr"])
    robust = want["margin"] >= 1e-6
    print("gammas 0.8 / 0.6, min_ratio 1e-3, 12 neighbours: %d candidates, %d decisions below the margin"
          % (want["candidate"].sum(), (~robust).sum()))
    assert (~robust).sum() <= 0.02 * len(robust) and 10 < want["candidate"].sum() < I.case_oracle("small_075")[0][
        "candidate"].sum()
    np.testing.assert_array_equal((sal != -1.0)[robust], want["candidate"][robust])
    # min_ratio 0 is Open3D's rule: the exactly planar fragment is decided by rounding, everything else as before
    zero, _ = _raw_saliency(ix, sal_r, min_ratio=0.0)
    base, _ = _raw_saliency(ix, sal_r)
    flat = np.zeros(len(pts), bool)
    flat[off[I.PLANAR]:off[I.PLANAR + 1]] = True
    assert zero[~flat].tobytes() == base[~flat].tobytes() and (base[flat] == -1.0).all()


def test_nms_on_planted_scores(gpu):
    A, B = K.clouds()[:2]
    pts, off = K.stack([A, B]), K.offsets([A, B])
    ix = _index(gpu, [A, B], K.R_CELL)
    # exact ties, zeros, negatives and NaN; radius 0.05 on the 0.075 index
    score = I.planted_scores(len(pts), 21)
    want = I.nms(pts, off, 0.05, I.MIN_NEIGHBORS, score)
    keep = _raw_nms(ix, 0.05, score)
    np.testing.assert_array_equal(keep, want["keep"])
    assert not keep[~(score > 0)].any() and keep.sum() > 50
    # balls short of min_neighbors: the planted outliers are alone, unbeaten, and not kept
    ones = _raw_nms(ix, 0.05, np.ones(len(pts)))
    np.testing.assert_array_equal(ones, I.nms(pts, off, 0.05, I.MIN_NEIGHBORS, np.ones(len(pts)))["keep"])
    sparse = K.radius_count(pts, off, 0.05) < I.MIN_NEIGHBORS
    assert sparse.sum() >= 30 and not ones[sparse].any()
    assert _raw_nms(ix, 0.05, np.ones(len(pts)), min_n=1)[sparse].any()
    # duplicated points and a lattice, scores tied exactly: only the lower row survives
    frags, r = K.ties_case()
    tix = _index(gpu, frags, r)
    ts = I.ties_scores(frags[0])
    tkeep = _raw_nms(tix, 0.05, ts, min_n=2)
    np.testing.assert_array_equal(tkeep, I.nms(frags[0], K.offsets(frags), 0.05, 2, ts)["keep"])
    _, first, inv = np.unique(frags[0], axis=0, return_index=True, return_inverse=True)
    copies = first[inv.reshape(-1)] != np.arange(len(frags[0]))
    assert not tkeep[copies].any() and tkeep.sum() > 5


def test_arguments_on_the_device(gpu):
    import torch
    from lib import _native as N
    L = N.lib()
    s = N.stream()
    ix = _index(gpu, [np.zeros((10, 3))], 0.05)
    sal = torch.empty(10, dtype=torch.float64, device=gpu)
    n_nbr = torch.empty(10, dtype=torch.int32, device=gpu)
    keep = torch.empty(10, dtype=torch.uint8, device=gpu)
    good = [N.ptr(ix["index"]), ix["ib"], N.ptr(ix["xyz"]), N.ptr(ix["off"]), 1, 10, 0.05, 0.05, 0.975, 0.975, 1e-6, 5,
            N.ptr(sal), N.ptr(n_nbr), s]
    assert L.mvr_iss_saliency(*good) == 0
    assert (n_nbr == 10).all() and (sal == -1.0).all()                 # ten coincident points: a zero covariance
    for at in (0, 2, 3, 12):
        args = list(good)
        args[at] = None
        assert L.mvr_iss_saliency(*args) == -1, at
    for at, v in ((1, ix["ib"] - 1), (7, 0.0500001), (8, 0.0), (9, 1.5), (10, 1.0), (11, 0)):
        args = list(good)
        args[at] = v
        assert L.mvr_iss_saliency(*args) == -1, at
    score = torch.ones(10, dtype=torch.float64, device=gpu)
    good = [N.ptr(ix["index"]), ix["ib"], N.ptr(ix["xyz"]), N.ptr(ix["off"]), 1, 10, 0.05, 0.05, 5, N.ptr(score),
            N.ptr(keep), s]
    assert L.mvr_radius_nms(*good) == 0
    assert keep.cpu().tolist() == [1] + [0] * 9                        # ten tied copies: the lowest row
    for at in (0, 2, 3, 9, 10):
        args = list(good)
        args[at] = None
        assert L.mvr_radius_nms(*args) == -1, at
    for at, v in ((1, ix["ib"] - 1), (7, 0.06), (8, 0)):
        args = list(good)
        args[at] = v
        assert L.mvr_radius_nms(*args) == -1, at


# ------------------------------------------------------------------------------------------- (d): the Python surface
def test_fo_iss_keypoints_and_select(gpu):
    import torch
    from lib.overlap import FragmentOverlap
    frags, r_index, sal_r, nms_r = I.case("clouds")
    want_s, want_n = I.case_oracle("clouds")
    fo = FragmentOverlap(frags, "3DMatch", radius=r_index)
    kp = fo.iss_keypoints(non_max_radius=nms_r)                        # salient_radius None: fo.r
    assert set(kp) == {"keep", "saliency", "n_nbr", "rows", "off"}
    assert kp["keep"].dtype == torch.bool and kp["saliency"].dtype == torch.float64
    assert kp["n_nbr"].dtype == torch.int32 and kp["rows"].dtype == torch.int64
    for k in ("keep", "saliency", "n_nbr"):
        assert tuple(kp[k].shape) == (fo.M,) and kp[k].device == fo.xyz.device, k
    assert kp["rows"].device == fo.xyz.device and isinstance(kp["off"], np.ndarray) and kp["off"].dtype == np.int64
    keep, rows = kp["keep"].cpu().numpy(), kp["rows"].cpu().numpy()
    assert (np.diff(rows) > 0).all() and rows.tolist() == np.flatnonzero(keep).tolist()
    assert kp["off"].tolist() == [0, int(keep[:fo.off[1]].sum()), int(keep.sum())] and kp["off"][-1] == len(rows) > 20
    _same_saliency("fo.iss_keypoints", kp["saliency"].cpu().numpy(), kp["n_nbr"].cpu().numpy(), want_s)
    robust = want_n["margin"] >= 1e-9
    np.testing.assert_array_equal(keep[robust], want_n["keep"][robust])
    # the defaults: salient fo.r, non-max 2/3 fo.r
    dflt = fo.iss_keypoints()
    assert dflt["saliency"].cpu().numpy().tobytes() == kp["saliency"].cpu().numpy().tobytes()
    own = I.nms(K.stack(frags), fo.off, 2.0 * fo.r / 3.0, 5, dflt["saliency"].cpu().numpy())
    np.testing.assert_array_equal(dflt["keep"].cpu().numpy(), own["keep"])
    with pytest.raises(ValueError, match="iss_keypoints: salient_radius"):
        fo.iss_keypoints(0.08)
    with pytest.raises(ValueError, match="iss_keypoints: min_neighbors"):
        fo.iss_keypoints(min_neighbors=0)
    # the keypoints as a cloud of their own: the method works on the selected object, an emptied one included
    fo2 = fo.select(kp["keep"])
    assert fo2.M == len(rows) and fo2.off.tolist() == kp["off"].tolist()
    assert fo2.parent_rows.cpu().tolist() == rows.tolist()
    kp2 = fo2.iss_keypoints(min_neighbors=1)
    pts2 = fo2.xyz.cpu().numpy()
    np.testing.assert_array_equal(kp2["n_nbr"].cpu().numpy(), K.radius_count(pts2, fo2.off, fo2.r))
    own2 = I.nms(pts2, fo2.off, 2.0 * fo2.r / 3.0, 1, kp2["saliency"].cpu().numpy())
    np.testing.assert_array_equal(kp2["keep"].cpu().numpy(), own2["keep"])
    fo3 = fo.select(torch.zeros(fo.M, dtype=torch.bool, device=gpu))
    kp3 = fo3.iss_keypoints()
    assert kp3["rows"].shape == (0,) and kp3["off"].tolist() == [0, 0, 0] and kp3["keep"].shape == (0,)


# -------------------------------------------------------------------------------------------------- (e): registration
def _rot_deg(Ra, Rb):
    return np.rad2deg(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


@functools.lru_cache(maxsize=None)
def _copy_fo():
    """tests/test_gpu_fpfh.py's full-copy case: index 0.075, oriented normals, compute_fpfh(0.075)"""
    from lib.overlap import FragmentOverlap
    src, tgt, Tt = I.copy_case()
    c = src.mean(0)
    fo = FragmentOverlap([src, tgt], "3DMatch", radius=I.COPY_R_INDEX)
    fo.estimate_normals(viewpoints=np.asarray([c, Tt[:3, :3] @ c + Tt[:3, 3]]))
    fo.compute_fpfh(I.COPY_R_INDEX)
    return fo


def test_registration_on_keypoints_recovers_the_full_copy(gpu):
    from lib.fpfh import match_features, match_keypoints, register_fgr, register_fpfh
    from lib.utils import RANSAC_DIST
    src, tgt, Tt = I.copy_case()
    c = src.mean(0)
    fo = _copy_fo()
    kp = fo.iss_keypoints(non_max_radius=I.COPY_NON_MAX)
    keep = kp["keep"].cpu().numpy()
    rep = I.repeated(src, tgt, Tt, keep)
    # the oracle gives 50 source keypoints of which 26 repeat (asserted in tests/test_iss_host.py); up to six NMS
    # decisions of the case are ties, so the GPU's counts may differ from those by a few: printed, not asserted
    print("keypoints %s of %s points, %d repeated" % (np.diff(kp["off"]).tolist(), np.diff(fo.off).tolist(), rep.sum()))
    base = register_fpfh(fo, [[0, 1]], seed=0)
    none = register_fpfh(fo, [[0, 1]], seed=0, keypoints=None)
    assert none["T"].tobytes() == base["T"].tobytes() and set(none) == set(base) == {"T", "fitness", "rmse",
                                                                                     "n_matches"}
    assert register_fgr(fo, [[0, 1]], keypoints=None)["T"].tobytes() == register_fgr(fo, [[0, 1]])["T"].tobytes()
    is_kp = [keep[:fo.off[1]], keep[fo.off[1]:]]
    for match in ("keypoints", "all"):
        rows = match_keypoints(fo.fpfh, fo.off, [[0, 1]], kp["rows"], kp["off"], True, match)[0].cpu().numpy()
        assert is_kp[0][rows[:, 0]].all() and (np.diff(rows[:, 0]) > 0).all()
        assert (is_kp[1][rows[:, 1]].all() if match == "keypoints" else (rows[:, 1] < len(tgt)).all())
        if match == "all":   # what the full matcher gives for those source rows where it agrees on mutuality
            every = match_features(fo.fpfh, fo.off, [[0, 1]], mutual=False)[0].cpu().numpy()
            one_way = match_keypoints(fo.fpfh, fo.off, [[0, 1]], kp["rows"], kp["off"], False, match)[0].cpu().numpy()
            np.testing.assert_array_equal(one_way, every[is_kp[0]])
        for name, f in (("register_fpfh", register_fpfh), ("register_fgr", register_fgr)):
            out = f(fo, [[0, 1]], seed=0, keypoints=kp, match=match)
            T = out["T"][0]
            dt = np.linalg.norm((T[:3, :3] @ c + T[:3, 3]) - (Tt[:3, :3] @ c + Tt[:3, 3]))
            dr = _rot_deg(T[:3, :3], Tt[:3, :3])
            print("%s(match=%r): %d matches of %s keypoints, fitness %.3f, rmse %.4f; off by %.4f m at the centroid, "
                  "%.3f deg" % (name, match, out["n_matches"][0], out["n_keypoints"][0].tolist(), out["fitness"][0],
                                out["rmse"][0], dt, dr))
            assert out["n_keypoints"].dtype == np.int64 and out["n_keypoints"].tolist() == [np.diff(kp["off"]).tolist()]
            assert out["n_matches"][0] == len(rows) and set(out) - set(base) >= {"n_keypoints"}
            assert dt <= RANSAC_DIST and dr <= 1.0
    # keypoints=True detects with the defaults
    auto = register_fpfh(fo, [[0, 1]], seed=0, keypoints=True)
    assert auto["n_keypoints"].tolist() == [np.diff(fo.iss_keypoints()["off"]).tolist()]
    with pytest.raises(ValueError, match="register_fpfh: match"):
        register_fpfh(fo, [[0, 1]], keypoints=True, match="mutual")


# ------------------------------------------------------------------------------------------ (f): the scene, the CLIs
def test_register_scene_with_keypoints(gpu):
    from lib.multiview import register_scene
    raw = O.scene4()[0]
    res = register_scene(raw, 0.025, seed=3, overlap_threshold=0.0, keypoints=True)
    fo = res["fo"]
    kp = fo.iss_keypoints()
    assert set(res["keypoints"]) == {"rows", "off"}
    assert res["keypoints"]["rows"].tolist() == kp["rows"].cpu().tolist() and res["keypoints"]["rows"].dtype == np.int64
    assert res["keypoints"]["off"].tolist() == kp["off"].tolist() and (np.diff(kp["off"]) > 5).all()
    print("register_scene(keypoints=True): keypoints per fragment %s of %s" % (np.diff(kp["off"]).tolist(),
                                                                             np.diff(fo.off).tolist()))
    assert np.isfinite(res["poses"]).all() and res["poses"].shape == (4, 4, 4)
    assert np.isfinite(res["pairs"]["T_coarse"]).all()
    opt = register_scene(raw, 0.025, seed=3, overlap_threshold=0.0, coarse="fgr",
                         keypoints={"match": "all", "non_max_radius": 0.035})
    assert np.isfinite(opt["poses"]).all() and len(opt["keypoints"]["rows"]) > len(kp["rows"])
    with pytest.raises(ValueError, match="keypoints"):
        register_scene(raw, 0.025, keypoints={"salient_radius": 0.08})


def test_the_two_scripts_with_keypoints(gpu, tmp_path, monkeypatch, capsys):
    from lib.ply import write_ply_xyz
    from lib.utils import load_config, read_trajectory
    from scripts.fuse_scene import read_poses
    from scripts.pairwise_demo import main as demo_main, parser as demo_parser
    from scripts.register_scene import main
    files = []
    for b, f in enumerate(O.scene4()[0]):
        files.append(str(tmp_path / ("frag_%d.ply" % b)))
        write_ply_xyz(files[-1], f[::2])
    out = str(tmp_path / "out")
    res = main(["--fragments"] + files + ["--out", out, "--keypoints", "iss", "--seed", "1"])
    printed = capsys.readouterr().out
    assert "registered 4 fragments" in printed
    assert ("keypoints (iss): per fragment: %s" % " ".join(str(int(v)) for v in np.diff(res["keypoints"]["off"]))) \
        in printed
    np.testing.assert_allclose(read_poses(out + "/poses.txt", 4), res["poses"], rtol=0, atol=1e-11)
    assert os.path.exists(out + "/traj.txt") and os.path.exists(out + "/scene.ply")
    with pytest.raises(SystemExit):
        main(["--fragments"] + files + ["--out", out, "--keypoints", "iss:0.08:0.05"])
    # pairwise_demo --fpfh --iss on the demo pair: no ground truth here, the counts are printed
    src, tgt = os.path.join(DEMO, "cloud_bin_0.ply"), os.path.join(DEMO, "cloud_bin_1.ply")
    monkeypatch.chdir(tmp_path)
    a = demo_parser().parse_args([DEMO_CFG, "--source_pc", src, "--target_pc", tgt, "--fpfh", "--iss"])
    T = demo_main(load_config(a.config), a)
    printed = capsys.readouterr().out
    print(printed)
    assert "ISS: " in printed and "T (source -> target)" in printed
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-9 and (T[3] == [0.0, 0.0, 0.0, 1.0]).all()
    _, traj = read_trajectory(str(tmp_path / "data/demo/pairwise/results/est_T.log"))
    np.testing.assert_allclose(traj[0], T, atol=1e-9)
    b = demo_parser().parse_args([DEMO_CFG, "--source_pc", src, "--target_pc", tgt, "--iss"])
    with pytest.raises(ValueError, match="--iss"):
        demo_main(load_config(b.config), b)
