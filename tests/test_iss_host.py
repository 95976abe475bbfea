"""CPU checks of the ISS keypoint detector's oracle (tests/iss_oracle.py), of the margins every case of
tests/test_gpu_iss.py is compared under, and of everything of the feature that needs no device: the argument checks of
FragmentOverlap.iss_keypoints, register_fpfh / register_fgr / register_scene(keypoints=...) and the two scripts, the
row mapping of lib.fpfh.keypoint_match_rows, and the empty-count and EINVAL conventions of mvr_iss_saliency and
mvr_radius_nms.

Margins.  The GPU accumulates in another order than numpy and may contract a * b + c, about 1e-15 relative in a
distance and 1e-13 in an eigenvalue ratio.  A distance is at least 1e-7 (relative) from its radius, an eigenvalue
ratio at least 1e-6 from its threshold (the smallest measured: 1.7e-5 on the registration case, 2.6e-4 elsewhere), so
n_nbr and the candidate set are compared exactly and without exclusions.  An NMS decision hangs on the gap to the
largest competing score (tests/iss_oracle.py says why that one is the measure of the decision); two close points
with the same neighbours have the same covariance up to rounding, so a few gaps are 0 or 1e-15: those decisions (gap
below 1e-9) are left out of the end-to-end comparison only, and their share is capped at 2 % of the candidates
(measured: 6 of 3189, 3 of 1146, 5 of 1146, 16 of 920, 6 of 3126).  The gap to the *closest* score of the ball, deciding
or not, is below 1e-9 far more often on randomly sampled clouds (118 of 3189, 55, 87 and 88 on the four cases; 10 of
3126 on the voxel centroids): it is printed, not capped, since a near tie below a clear maximum flips nothing."""
import inspect
import os
import types

import numpy as np
import pytest

from conftest import PKG
import icp_oracle as O
import iss_oracle as I
import knn_oracle as K

LIB = os.path.join(PKG, "libmvreg_hip.so")
MARGIN_RADIUS = 1e-7
MARGIN_SALIENCY = 1e-6
MARGIN_NMS = 1e-9
CAP_TIES = 0.02


# ---------------------------------------------------------------------------------------------------------- the oracle
def test_a_flat_patch_has_no_candidate_and_a_bump_has_its_keypoint():
    flat = I.bump_patch(bump=0.0)
    off = K.offsets([flat])
    s, n = I.iss(flat, off, 0.075, 0.05)
    assert (s["n_nbr"] >= I.MIN_NEIGHBORS).all() and not s["candidate"].any() and (s["saliency"] == -1.0).all()
    assert not n["keep"].any()
    # without the floor rounding noise decides: Open3D's rule makes candidates of a plane
    assert I.saliency(flat, off, 0.075, min_ratio=0.0)["candidate"].any()
    bump = I.bump_patch()
    s, n = I.iss(bump, off, 0.075, 0.05)
    kp = bump[n["keep"]]
    assert 1 <= len(kp) <= 8 and (np.linalg.norm(kp[:, :2], axis=1) < 0.12).all(), kp
    assert s["saliency"][n["keep"]].min() > 0 and (s["saliency"][~s["candidate"]] == -1.0).all()
    # the strongest response sits on the bump itself
    assert np.linalg.norm(bump[np.argmax(s["saliency"]), :2]) < 0.06


def test_a_rigid_motion_keeps_the_keypoint_set():
    A = K.clouds()[0]
    off = K.offsets([A])
    T = O.rigid([0.3, -1.0, 0.5], 37.0, [0.4, -0.2, 0.1])
    moved = A @ T[:3, :3].T + T[:3, 3]
    s0, n0 = I.iss(A, off, 0.075, 0.05)
    s1, n1 = I.iss(moved, off, 0.075, 0.05)
    np.testing.assert_array_equal(s0["n_nbr"], s1["n_nbr"])
    np.testing.assert_array_equal(s0["candidate"], s1["candidate"])
    np.testing.assert_allclose(s1["eig"], s0["eig"], rtol=0, atol=1e-12 * s0["eig"].max())
    robust = n0["margin"] >= MARGIN_NMS
    np.testing.assert_array_equal(n0["keep"][robust], n1["keep"][robust])
    assert n0["keep"].sum() >= 20


def test_nms_rules_on_a_line_of_points():
    x = np.zeros((7, 3))
    x[:, 0] = [0.0, 0.01, 0.02, 0.03, 0.5, 0.51, 0.51]
    off = K.offsets([x])
    out = I.nms(x, off, 0.025, 1, [1.0, 2.0, 2.0, -1.0, np.nan, 3.0, 3.0])
    # the tie goes to the lower row, a duplicate included; a NaN neither survives nor suppresses
    assert out["keep"].tolist() == [False, True, False, False, False, True, False]
    assert out["margin"][1] == 0.0 and out["margin"][5] == 0.0 and np.isinf(out["margin"][3])
    # a ball short of min_neighbors keeps nothing, whatever the score
    assert I.nms(x, off, 0.025, 4, [1.0, 2.0, 2.0, 5.0, 9.0, 3.0, 3.0])["keep"].tolist() == [False] * 7
    assert I.nms(x, off, 0.025, 3, [1.0, 2.0, 2.0, 5.0, 9.0, 3.0, 3.0])["keep"].tolist() == \
        [False, False, False, True, True, False, False]
    # fragments do not see each other
    two = I.nms(np.concatenate([x, x]), K.offsets([x, x]), 0.025, 1, [1.0, 2.0, 2.0, -1.0, np.nan, 3.0, 3.0] * 2)
    assert two["keep"].tolist() == out["keep"].tolist() * 2


# ------------------------------------------------------------------------------------------- margins of the GPU cases
@pytest.mark.parametrize("name", I.CASES)
def test_every_decision_of_the_gpu_cases_has_its_margin(name):
    frags, r_index, sal_r, nms_r = I.case(name)
    s, n = I.case_oracle(name)
    n_cand = int(s["candidate"].sum())
    ties, near = int((n["margin"] < MARGIN_NMS).sum()), int((n["nearest"] < MARGIN_NMS).sum())
    print("%s: %d points, %d candidates, %d keypoints; radius margins %.3g / %.3g, smallest saliency margin %.3g; "
          "NMS decisions within 1e-9 of the deciding score %d (%.2f %%), of the closest score %d (%.2f %%)"
          % (name, len(s["candidate"]), n_cand, int(n["keep"].sum()), s["radius_margin"], n["radius_margin"],
             s["margin"].min(), ties, 100.0 * ties / n_cand, near, 100.0 * near / n_cand))
    assert 0 < sal_r <= r_index and 0 < nms_r <= r_index
    assert s["radius_margin"] >= MARGIN_RADIUS and n["radius_margin"] >= MARGIN_RADIUS
    assert s["margin"].min() >= MARGIN_SALIENCY                     # every point: nothing is left out of (a)
    assert ties <= CAP_TIES * n_cand
    assert n_cand > 100 and n["keep"].sum() > 10
    if name != "clouds":
        off = K.offsets(frags)
        short = np.flatnonzero(np.diff(off) < I.MIN_NEIGHBORS)
        assert short.tolist() == [0, 1, 2, 3]
        assert (s["saliency"][:off[4]] == -1.0).all() and (s["saliency"][off[I.PLANAR]:off[I.PLANAR + 1]] == -1.0).all()
        assert (s["n_nbr"][off[I.PLANAR]:off[I.PLANAR + 1]] >= I.MIN_NEIGHBORS).any()   # rejected as flat, not as sparse


def test_planted_score_cases_have_their_radius_margin():
    A, B = K.clouds()[:2]
    pts, off = K.stack([A, B]), K.offsets([A, B])
    out = I.nms(pts, off, 0.05, I.MIN_NEIGHBORS, I.planted_scores(len(pts), 21))
    assert out["radius_margin"] >= MARGIN_RADIUS and 50 < out["keep"].sum() < out["decided"].sum()
    assert (out["margin"][out["decided"]] == 0).sum() > 20                           # exact ties do occur
    # points alone in their ball: positive, unbeaten, and still not kept
    alone = I.nms(pts, off, 0.05, I.MIN_NEIGHBORS, np.ones(len(pts)))
    sparse = K.radius_count(pts, off, 0.05) < I.MIN_NEIGHBORS
    assert sparse.sum() >= 30 and not alone["keep"][sparse].any() and not alone["decided"][sparse].any()
    frags, r = K.ties_case()
    t = I.nms(frags[0], K.offsets(frags), 0.05, 2, I.ties_scores(frags[0]))
    assert t["radius_margin"] >= MARGIN_RADIUS
    # of the three stored copies of a point at most the lowest row survives
    _, first, inv = np.unique(frags[0], axis=0, return_index=True, return_inverse=True)
    copies = first[inv.reshape(-1)] != np.arange(len(frags[0]))
    assert copies.sum() == 100 and not t["keep"][copies].any() and t["keep"].sum() > 5


def test_the_registration_case_has_enough_repeated_keypoints():
    src, tgt, Tt = I.copy_case()
    s, n = I.copy_oracle()
    keep = n["keep"]
    rep = I.repeated(src, tgt, Tt, keep)
    n_cand = int(s["candidate"].sum())
    print("full copy at non-max radius %g: %d / %d keypoints, %d source keypoints land on a target keypoint; "
          "smallest saliency margin %.3g, %d of %d NMS decisions within 1e-9"
          % (I.COPY_NON_MAX, keep[:len(src)].sum(), keep[len(src):].sum(), rep.sum(), s["margin"].min(),
             (n["margin"] < MARGIN_NMS).sum(), n_cand))
    assert keep[:len(src)].sum() >= I.COPY_MIN_KEYPOINTS and rep.sum() >= I.COPY_MIN_REPEATED
    assert s["radius_margin"] >= MARGIN_RADIUS and n["radius_margin"] >= MARGIN_RADIUS
    assert s["margin"].min() >= MARGIN_SALIENCY and (n["margin"] < MARGIN_NMS).sum() <= CAP_TIES * n_cand
    # the matches the oracle's descriptors give on those keypoints: enough for a 3-point RANSAC to be no matter of
    # luck, and with the inlier share Fast Global Registration needs (tens of percent)
    for match in ("keypoints", "all"):
        rows, inlier = I.copy_matches(match)
        print("match=%r: %d mutual matches, %d inliers" % (match, len(rows), inlier.sum()))
        assert keep[rows[:, 0]].all() and (match == "all" or keep[len(src) + rows[:, 1]].all())
        assert inlier.sum() >= 20 and inlier.mean() >= 0.5


# -------------------------------------------------------------------------------------------------- argument helpers
def test_iss_keypoints_arguments():
    from lib import overlap as V
    sig = inspect.signature(V.FragmentOverlap.iss_keypoints).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == list(V.ISS_DEFAULTS.items()) == [
        ("salient_radius", None), ("non_max_radius", None), ("gamma_21", 0.975), ("gamma_32", 0.975),
        ("min_neighbors", 5), ("min_ratio", 1e-6)]
    assert V._iss_arguments(None, None, 0.975, 0.975, 5, 1e-6, 0.075) == (0.075, 2.0 * 0.075 / 3.0, 0.975, 0.975, 5, 1e-6)
    assert V._iss_arguments(0.06, 0.075, 1, 1.0, 1, 0, 0.075) == (0.06, 0.075, 1.0, 1.0, 1, 0.0)
    good = dict(salient_radius=None, non_max_radius=None, gamma_21=0.975, gamma_32=0.975, min_neighbors=5,
                min_ratio=1e-6)
    bad = [("salient_radius", v) for v in (0.0, -0.1, 0.0751, float("nan"), "0.05", True)] + \
          [("non_max_radius", v) for v in (0.0, 0.08, float("nan"))] + \
          [(g, v) for g in ("gamma_21", "gamma_32") for v in (0.0, -0.5, 1.0001, float("nan"), None)] + \
          [("min_neighbors", v) for v in (0, -1, 2.5, True, None)] + \
          [("min_ratio", v) for v in (-1e-9, 1.0, 2.0, float("nan"), None)]
    for key, v in bad:
        with pytest.raises(ValueError, match="iss_keypoints: %s" % key):
            V._iss_arguments(r=0.075, **dict(good, **{key: v}))


def _fake_fo(M=10, B=2):
    import torch
    return types.SimpleNamespace(fpfh=torch.zeros(M, 33), M=M, B=B, off=np.array([0, 4, M]), device="cpu")


def test_keypoint_arguments_of_the_registrations_raise_before_any_device_work():
    import torch
    from lib import fpfh as F
    for f in (F.register_fpfh, F.register_fgr):
        sig = inspect.signature(f).parameters
        assert sig["keypoints"].default is None and sig["match"].default == "keypoints"
    assert F.KEYPOINT_MATCH == ("keypoints", "all")
    assert F._keypoint_arguments("f", None, "all") is None and F._keypoint_arguments("f", True, "keypoints") is True
    rows, off = F._keypoint_arguments("f", {"rows": torch.tensor([1, 5, 7]), "off": [0, 1, 3], "keep": None}, "all", 2)
    assert rows.tolist() == [1, 5, 7] and off.tolist() == [0, 1, 3] and off.dtype == np.int64
    fo = _fake_fo()
    bad = [{"keypoints": True, "match": "mutual"}, {"keypoints": "iss"}, {"keypoints": False}, {"keypoints": {}},
           {"keypoints": {"rows": torch.tensor([1, 5])}}, {"keypoints": {"rows": [1, 5], "off": [0, 1, 2]}},
           {"keypoints": {"rows": torch.tensor([1.0, 5.0]), "off": [0, 1, 2]}},
           {"keypoints": {"rows": torch.tensor([1, 5]), "off": [0, 1, 3]}},          # does not end at K
           {"keypoints": {"rows": torch.tensor([1, 5]), "off": [0, 2, 1, 2]}},       # not the fragments' count
           {"keypoints": {"rows": torch.tensor([1, 5]), "off": [0, 2]}}]
    for kw in bad:
        for f in (F.register_fpfh, F.register_fgr):
            with pytest.raises(ValueError, match="%s: (match|keypoints)" % f.__name__):
                f(fo, [[0, 1]], **kw)


def test_keypoints_argument_of_register_scene():
    from lib import multiview as MV
    assert inspect.signature(MV.register_scene).parameters["keypoints"].default is None
    assert MV._keypoints_arguments(None) is None
    full = {"salient_radius": None, "non_max_radius": None, "gamma_21": 0.975, "gamma_32": 0.975, "min_neighbors": 5,
            "min_ratio": 1e-6, "match": "keypoints"}
    assert MV._keypoints_arguments(True, 0.075) == full and MV._keypoints_arguments({}, 0.075) == full
    got = MV._keypoints_arguments({"match": "all", "non_max_radius": 0.035, "min_neighbors": 7, "gamma_21": 1}, 0.075)
    assert got == dict(full, match="all", non_max_radius=0.035, min_neighbors=7, gamma_21=1.0)
    for bad in (False, "iss", 3, {"match": "mutual"}, {"radius": 0.05}, {"salient_radius": 0.08},
                {"non_max_radius": 0.0}, {"gamma_32": 1.5}, {"min_neighbors": 0}, {"min_ratio": 1.0}):
        with pytest.raises(ValueError):
            MV._keypoints_arguments(bad, 0.075)
    with pytest.raises(ValueError, match="init replaces"):
        MV._keypoints_arguments(True, 0.075, init=np.tile(np.eye(4), (1, 1, 1)))
    # the checks come before any device work: no fragment is looked at
    with pytest.raises(ValueError, match="keypoints"):
        MV.register_scene([None, None], 0.025, keypoints={"match": "mutual"})
    with pytest.raises(ValueError, match="keypoints"):
        MV.register_scene([None, None], 0.025, keypoints=True, init=np.tile(np.eye(4), (1, 1, 1)))


def test_keypoint_options_of_the_two_scripts():
    from scripts import pairwise_demo as D
    from scripts import register_scene as S
    assert S.parse_keypoints("iss") == {}
    assert S.parse_keypoints("iss:0.075:0.035") == {"salient_radius": 0.075, "non_max_radius": 0.035}
    for bad in ("", "harris", "iss:0.05", "iss:a:b", "iss:0.05:0.04:0.03", "ISS"):
        with pytest.raises(ValueError, match="--keypoints must be"):
            S.parse_keypoints(bad)
    ap = S.parser()
    base = ["--fragments", "a.ply", "b.ply", "--out", "o"]
    assert S.check_args(ap, ap.parse_args(base)).keypoints is None
    a = S.check_args(ap, ap.parse_args(base + ["--keypoints", "iss"]))
    assert a.keypoints["match"] == "keypoints" and a.keypoints["salient_radius"] is None
    a = S.check_args(ap, ap.parse_args(base + ["--keypoints", "iss:0.06:0.04", "--coarse", "fgr"]))
    assert (a.keypoints["salient_radius"], a.keypoints["non_max_radius"]) == (0.06, 0.04)
    for extra in (["--keypoints", "iss:0.08:0.05"], ["--keypoints", "iss:0.05:0"], ["--keypoints", "sift"],
                  ["--keypoints", "iss", "--init", "traj.txt"]):                       # 0.08 > 3 voxels of 0.025
        with pytest.raises(SystemExit):
            S.check_args(ap, ap.parse_args(base + extra))
    dp = D.parser()
    assert dp.parse_args(["cfg.yaml"]).iss is False
    assert D.check_args(dp.parse_args(["cfg.yaml", "--fpfh", "--iss"])).iss is True
    assert D.check_args(dp.parse_args(["cfg.yaml", "--fpfh", "--fgr", "--iss"])).iss is True
    with pytest.raises(ValueError, match="--iss .* needs --fpfh"):
        D.check_args(dp.parse_args(["cfg.yaml", "--iss"]))


# ---------------------------------------------------------------------------------------------------- the row mapping
def test_keypoint_matches_map_back_to_fragment_rows():
    import torch
    from lib.fpfh import keypoint_match_rows
    off = np.array([0, 10, 10, 25])                      # fragments of 10, 0 and 15 points
    kp_rows = torch.tensor([2, 5, 9, 10, 17, 24])        # rows of the stacked cloud, ascending
    kp_off = np.array([0, 3, 3, 6])
    pairs = [[0, 2], [2, 0], [1, 2]]
    among = [torch.tensor([[0, 2], [2, 0]]), torch.tensor([[1, 1], [2, 2]]), torch.zeros(0, 2, dtype=torch.int64)]
    got = keypoint_match_rows(among, pairs, off, kp_rows, kp_off, "keypoints")
    assert [g.tolist() for g in got] == [[[2, 14], [9, 0]], [[7, 5], [14, 9]], []]
    assert all(g.dtype == torch.int64 and tuple(g.shape[1:]) == (2,) for g in got)
    # 'all': the target column already is a row within the target fragment
    to_all = [torch.tensor([[0, 13], [1, 0]]), torch.tensor([[0, 9]]), torch.zeros(0, 2, dtype=torch.int64)]
    got = keypoint_match_rows(to_all, pairs, off, kp_rows, kp_off, "all")
    assert [g.tolist() for g in got] == [[[2, 13], [5, 0]], [[0, 9]], []]
    with pytest.raises(ValueError, match="match must be"):
        keypoint_match_rows(to_all, pairs, off, kp_rows, kp_off, "mutual")


# ------------------------------------------------------------------------------------------- the ABI without a GPU
_Z = None


def _sal(L, M=0, B=2, r=0.05, radius=0.05, g21=0.975, g32=0.975, ratio=1e-6, nb=5):
    return L.mvr_iss_saliency(_Z, 0, _Z, _Z, B, M, r, radius, g21, g32, ratio, nb, _Z, _Z, _Z)


def _nms(L, M=0, B=2, r=0.05, radius=0.05, nb=5):
    return L.mvr_radius_nms(_Z, 0, _Z, _Z, B, M, r, radius, nb, _Z, _Z, _Z)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")
def test_entry_points_without_a_device():
    from lib import _native
    L = _native.lib()
    assert "mvr_iss_saliency" in _native.EXPORTS and "mvr_radius_nms" in _native.EXPORTS
    nan = float("nan")
    # M == 0: MVR_OK with NULL pointers
    assert _sal(L) == 0 and _nms(L) == 0
    assert _sal(L, radius=0.01, g21=1.0, g32=1.0, ratio=0.0, nb=1) == 0 and _nms(L, radius=0.01, nb=1) == 0
    # scalars are checked before the empty short-cut
    for f in (_sal, _nms):
        assert f(L, M=-1) == -1 and f(L, M=1 << 31) == -1 and f(L, B=0) == -1 and f(L, B=1 << 15) == -1
        assert f(L, r=0.0) == -1 and f(L, r=nan) == -1 and f(L, radius=0.0) == -1 and f(L, radius=-0.01) == -1
        assert f(L, radius=0.0500001) == -1 and f(L, radius=nan) == -1 and f(L, nb=0) == -1 and f(L, nb=-3) == -1
        assert f(L, M=10) == -1                                   # with points every pointer is needed
    for g in ("g21", "g32"):
        for v in (0.0, -0.1, 1.0000001, nan):
            assert _sal(L, **{g: v}) == -1, (g, v)
    for v in (-1e-12, 1.0, 1.5, nan):
        assert _sal(L, ratio=v) == -1, v
