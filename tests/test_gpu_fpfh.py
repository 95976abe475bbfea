"""GPU FPFH descriptors (csrc/fpfh.hip mvr_compute_fpfh, FragmentOverlap.compute_fpfh), the ragged feature matcher
(csrc/feat_match.hip mvr_feat_match, lib/fpfh.py) and the weights-free coarse registration built on them
(lib.fpfh.register_fpfh, scripts/pairwise_demo.py --fpfh) against the numpy oracle (tests/fpfh_oracle.py).

Tolerances.  The oracle runs on the GPU's own points and normals.  SPFH comes from integer counts, so on the rows
the oracle calls safe (no feature within 1e-9 bins of a bin edge, no undecided role swap) only the final division and
rounding can differ: one fp32 ulp of the oracle's fp32-rounded value.  FPFH is accumulated in fp64 in another order
(about 1e-13 relative), which moves a round-to-nearest by at most one ulp.  The shares of rows left out are printed and
capped (fpfh_oracle.CAP_*, asserted on the CPU by test_fpfh_host.py); the random shapes leave out none.
The matcher's indices are not compared (flat regions hold many identical descriptors): the chosen row's fp64 distance
must be at most the oracle's minimum x (1 + 1e-5) + 1e-4, the fp32 accumulation bound for 64 terms of magnitude
<= 200^2, and dist2 within the same bound of it."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
import icp_oracle as O
import fpfh_oracle as FO

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
DEMO = os.path.join(GOLDEN, "demo")
DEMO_CFG = os.path.join(GOLDEN, "configs", "pairwise_registration", "demo", "config.yaml")


def _split(fo, x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    return [x[fo.off[b]:fo.off[b + 1]] for b in range(fo.B)]


def _raw_fpfh(fo, radius):
    """mvr_compute_fpfh on sentinel-filled output buffers -> (fpfh [M,33], spfh [M,33]) numpy"""
    import torch
    from lib import _native as N
    L = N.lib()
    out = torch.full((fo.M, 33), SENTINEL, dtype=torch.float32, device=fo.device)
    spfh = torch.full((fo.M, 33), SENTINEL, dtype=torch.float32, device=fo.device)
    ws_b = L.mvr_compute_fpfh_workspace_bytes(fo.M)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=fo.device)
    N.check(L.mvr_compute_fpfh(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.normals),
                               N.ptr(fo.off_dev), fo.B, fo.M, fo.r, radius, N.ptr(out), N.ptr(spfh), N.ptr(ws), ws_b,
                               N.stream()), "mvr_compute_fpfh")
    return out.cpu().numpy(), spfh.cpu().numpy()


def _compare(what, got_f, got_s, want, cap_s, cap_f):
    """every row written; on the safe rows both histograms within one fp32 ulp of the oracle's rounded value"""
    assert got_f.shape == got_s.shape == (sum(len(w["k"]) for w in want), 33)
    assert not np.any(got_f == SENTINEL) and not np.any(got_s == SENTINEL)
    assert np.isfinite(got_f).all() and np.isfinite(got_s).all()
    at = 0
    for b, w in enumerate(want):
        n = len(w["k"])
        f, s = got_f[at:at + n], got_s[at:at + n]
        at += n
        if n == 0:
            continue
        safe_s, safe_f = ~w["unsafe_spfh"], ~w["unsafe_fpfh"]
        us = FO.ulps32(s, w["spfh"]).max(1)
        uf = FO.ulps32(f, w["fpfh"]).max(1)
        print("%s, fragment %d: %d rows, left out SPFH %.4f FPFH %.4f; largest difference on the others %.3g / %.3g "
              "ulp; rows off by more than an ulp among those left out: %d / %d"
              % (what, b, n, (~safe_s).mean(), (~safe_f).mean(), us[safe_s].max() if safe_s.any() else 0.0,
                 uf[safe_f].max() if safe_f.any() else 0.0, int((us[~safe_s] > 1).sum()),
                 int((uf[~safe_f] > 1).sum())))
        assert (~safe_s).mean() <= cap_s and (~safe_f).mean() <= cap_f
        assert (us[safe_s] <= 1.0).all() and (uf[safe_f] <= 1.0).all()
        zero = w["k"] == 0
        assert not s[zero].any() and not f[zero].any()


# -------------------------------------------------------------------------------------------------------- the scene
@functools.lru_cache(maxsize=None)
def _scene_fo():
    """fragments 0 and 1 of the scene on an index of cell 0.075, normals oriented to the fragments' means"""
    from lib.overlap import FragmentOverlap
    fo = FragmentOverlap([O.scene4()[0][b] for b in FO.SCENE_FRAGS], "FCGF", 0.025)
    fo.estimate_normals(viewpoints=np.asarray([f.mean(0) for f in _split(fo, fo.xyz)]))
    return fo


@pytest.mark.parametrize("radius", FO.SCENE_RADII)
def test_scene_fpfh_matches_oracle(gpu, radius):
    fo = _scene_fo()
    assert fo.r == 3 * 0.025 and abs(fo.max_points - 2600) < 200
    got_f, got_s = _raw_fpfh(fo, radius)
    want = FO.fpfh_batch(_split(fo, fo.xyz), _split(fo, fo.normals), radius)
    _compare("scene, radius %g" % radius, got_f, got_s, want, FO.CAP_SPFH, FO.CAP_FPFH)
    has = np.concatenate([w["k"] for w in want]) > 0
    np.testing.assert_allclose(got_f[has].astype(np.float64).sum(1), 600.0, rtol=0, atol=1e-3)
    # FragmentOverlap.compute_fpfh: the same call, stored on the object
    assert fo.compute_fpfh(radius).cpu().numpy().tobytes() == got_f.tobytes() and fo.fpfh.dtype.is_floating_point
    assert tuple(fo.fpfh.shape) == (fo.M, 33) and fo.fpfh.device == fo.xyz.device


# ------------------------------------------------------------------------------------------------- awkward shapes
def _small_fo(frags, normals):
    import torch
    from lib.overlap import FragmentOverlap
    fo = FragmentOverlap(frags, "3DMatch", radius=FO.SMALL_R_INDEX)
    fo.normals = torch.from_numpy(np.concatenate(normals).reshape(-1, 3)).to(fo.device).contiguous()
    return fo


def test_fpfh_on_small_shapes_in_one_batch(gpu):
    frags, normals = FO.small_case()
    fo = _small_fo(frags, normals)
    assert tuple(np.diff(fo.off)) == FO.SMALL_SIZES and fo.r == FO.SMALL_R_INDEX
    for radius in FO.SMALL_RADII:                                               # radius == r_index, radius < r_index
        got_f, got_s = _raw_fpfh(fo, radius)
        want = FO.fpfh_batch(frags, normals, radius)
        _compare("small shapes, radius %g" % radius, got_f, got_s, want, 0.0, 0.0)     # nothing is left out
        per = _split(fo, got_f)
        assert not per[1].any()                                                 # one point: no neighbour
        assert want[6]["k"][-1] >= 1 and want[6]["k"][-2] >= 1                  # the coincident pair counts in k
        # a fragment's rows do not depend on the fragments around it
        for b in (6, 7):
            alone = _small_fo([frags[b]], [normals[b]])
            one_f, one_s = _raw_fpfh(alone, radius)
            assert one_f.tobytes() == per[b].tobytes() and one_s.tobytes() == _split(fo, got_s)[b].tobytes()


# ------------------------------------------------------------------------------------------------------ the matcher
def _check_matches(what, F, off, pairs, idx, dist2, qoff):
    F64 = F.astype(np.float64)
    worst_r, worst_d = 0.0, 0.0
    for p, (a, b) in enumerate(pairs):
        Fq, Ft = F64[off[a]:off[a + 1]], F64[off[b]:off[b + 1]]
        got, d2 = idx[qoff[p]:qoff[p + 1]], dist2[qoff[p]:qoff[p + 1]].astype(np.float64)
        assert len(got) == len(Fq)
        if len(Fq) == 0:
            continue
        if len(Ft) == 0:
            assert (got == -1).all(), (what, p)                                 # an empty target
            continue
        assert (got >= 0).all() and (got < len(Ft)).all(), (what, p)
        best, _ = FO.nearest_feature(Fq, Ft)
        mine = ((Fq - Ft[got]) ** 2).sum(1)
        assert (mine <= best * (1 + 1e-5) + 1e-4).all(), (what, p, (mine - best).max())
        assert (np.abs(d2 - mine) <= mine * 1e-5 + 1e-4).all(), (what, p, np.abs(d2 - mine).max())
        # among the exact duplicates of the chosen row, the smallest index
        _, first, inv = np.unique(Ft, axis=0, return_index=True, return_inverse=True)
        assert (first[inv.reshape(-1)[got]] == got).all(), (what, p)
        worst_r, worst_d = max(worst_r, (mine - best).max()), max(worst_d, np.abs(d2 - mine).max())
    print("%s: %d pairs, %d queries; chosen - minimum at most %.3g, |dist2 - fp64| at most %.3g"
          % (what, len(pairs), int(qoff[-1]), worst_r, worst_d))


MATCH_SIZES = (0, 1, 2, 65, 1025)


@pytest.mark.parametrize("C", [1, 32, 33, 64])
def test_matcher_on_random_ragged_fragments(gpu, C):
    """every ordered pair of the five sizes, empty queries and empty targets among them; values in [0, 100] on a
    grid of 1/4 so that exact ties occur, and every seventh row of the larger fragments a copy of row 0"""
    import torch
    from lib.fpfh import feat_match
    rng = np.random.default_rng(10 + C)
    off = np.concatenate([[0], np.cumsum(MATCH_SIZES)]).astype(np.int64)
    F = (rng.integers(0, 401, (off[-1], C)) / 4.0).astype(np.float32)
    for b in (3, 4):
        F[off[b] + 7:off[b + 1]:7] = F[off[b]]
    pairs = np.asarray([(a, b) for a in range(5) for b in range(5)])
    idx, dist2, qoff = feat_match(torch.from_numpy(F).to(gpu), off, pairs)
    assert idx.dtype == torch.int32 and dist2.dtype == torch.float32 and len(idx) == qoff[-1] == 5 * off[-1]
    _check_matches("random, C = %d" % C, F, off, pairs, idx.cpu().numpy(), dist2.cpu().numpy(), qoff)


def test_matcher_on_scene_fpfh_and_mutual_filter(gpu):
    from lib.fpfh import feat_match, match_features
    fo = _scene_fo()
    F = fo.compute_fpfh(0.075)
    pairs = np.asarray([(0, 1), (1, 0), (1, 1)])
    idx, dist2, qoff = feat_match(F, fo.off, pairs)
    idx, dist2 = idx.cpu().numpy(), dist2.cpu().numpy()
    _check_matches("scene FPFH", F.cpu().numpy(), fo.off, pairs, idx, dist2, qoff)
    own = idx[qoff[2]:qoff[3]]                                                  # a fragment against itself
    assert (dist2[qoff[2]:qoff[3]] == 0).all() and (own <= np.arange(len(own))).all()
    # the mutual filter: the same filter applied to the GPU's own two index arrays
    st, ts = idx[qoff[0]:qoff[1]], idx[qoff[1]:qoff[2]]
    src = np.arange(len(st))
    want = np.stack([src, st], 1)[ts[st] == src]
    got = match_features(F, fo.off, pairs[:1])
    assert len(got) == 1 and got[0].dtype.is_floating_point is False
    np.testing.assert_array_equal(got[0].cpu().numpy(), want)
    every = match_features(F, fo.off, pairs[:2], mutual=False)
    np.testing.assert_array_equal(every[0].cpu().numpy(), np.stack([src, st], 1))
    np.testing.assert_array_equal(every[1].cpu().numpy(), np.stack([np.arange(len(ts)), ts], 1))
    print("scene FPFH: %d of %d source rows have a mutual match" % (len(want), len(st)))
    assert 0 < len(want) < len(st)


def test_match_features_with_empty_fragments(gpu):
    import torch
    from lib.fpfh import match_features
    rng = np.random.default_rng(3)
    off = np.asarray([0, 0, 5, 5, 70])
    F = torch.from_numpy(rng.random((70, 33)).astype(np.float32)).to(gpu)
    got = match_features(F, off, [[0, 1], [1, 0], [1, 3], [3, 3], [2, 0]])
    assert [len(g) for g in got][:2] == [0, 0] and len(got[4]) == 0 and 1 <= len(got[2]) <= 5
    np.testing.assert_array_equal(got[3].cpu().numpy(), np.stack([np.arange(65)] * 2, 1))


# ------------------------------------------------------------------------------------------------------- end to end
def _rot_deg(Ra, Rb):
    return np.rad2deg(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def test_register_fpfh_recovers_a_full_copy_and_feeds_icp(gpu):
    """icp_oracle.full_copy_case with the viewpoint moved too: the target is fragment 0's centroids moved by a known
    motion plus 500 distractors, shuffled.  The translation error is measured at the source's centroid (where the
    fragment is, not at the frame's origin a few metres away)."""
    from lib.fpfh import correspondences, match_features, register_fpfh
    from lib.icp import icp_refine
    from lib.overlap import FragmentOverlap
    from lib.utils import RANSAC_DIST, run_ransac_batch
    src = O.scene4_centroids()[0]
    tgt, Tt, _ = O.full_copy_case(src)
    c = src.mean(0)
    fo = FragmentOverlap([src, tgt], "3DMatch", radius=0.075)
    fo.estimate_normals(viewpoints=np.asarray([c, Tt[:3, :3] @ c + Tt[:3, 3]]))
    fo.compute_fpfh(0.075)
    out = register_fpfh(fo, [[0, 1]], seed=0)
    T = out["T"][0]
    dt = np.linalg.norm((T[:3, :3] @ c + T[:3, 3]) - (Tt[:3, :3] @ c + Tt[:3, 3]))
    dr = _rot_deg(T[:3, :3], Tt[:3, :3])
    print("register_fpfh: %d mutual matches of %d points, fitness %.3f, rmse %.4f; off by %.4f m at the centroid, "
          "%.3f deg" % (out["n_matches"][0], len(src), out["fitness"][0], out["rmse"][0], dt, dr))
    assert set(out) == {"T", "fitness", "rmse", "n_matches"} and out["T"].shape == (1, 4, 4)
    assert dt <= RANSAC_DIST and dr <= 1.0
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-9
    # bit for bit what run_ransac_batch gives on the same correspondences and seed
    matches = match_features(fo.fpfh, fo.off, [[0, 1]])
    assert len(matches[0]) == out["n_matches"][0]
    xs, xt = correspondences(fo, [[0, 1]], matches)
    by_hand = run_ransac_batch(xs, xt, [len(matches[0])], seed=0)
    assert by_hand.tobytes() == out["T"].tobytes()
    assert register_fpfh(fo, [[0, 1]], seed=0)["T"].tobytes() == out["T"].tobytes()
    # the ICP refinement from it reaches test_gpu_icp.py's bound for this case
    ref = icp_refine(fo, [[0, 1]], out["T"], max_dist=0.05, max_iters=30, tol_fitness=0.0, tol_rmse=0.0)
    print("icp_refine from it: |T - T_true| %.3g, rmse %.3g" % (np.abs(ref["T"][0] - Tt).max(), ref["rmse"][0]))
    np.testing.assert_allclose(ref["T"][0], Tt, rtol=0, atol=1e-9)
    assert ref["n_corr"][0] == len(src) and ref["fitness"][0] == 1.0 and ref["rmse"][0] < 1e-9


def test_register_fpfh_without_matches(gpu):
    """a pair with an empty fragment: no match, the identity"""
    from lib.fpfh import register_fpfh
    frags, normals = FO.small_case()
    fo = _small_fo(frags[:5], normals[:5])
    fo.compute_fpfh()
    out = register_fpfh(fo, [[0, 4], [4, 0], [4, 4]])
    assert out["n_matches"].tolist() == [0, 0, 63]
    np.testing.assert_array_equal(out["T"][:2], np.tile(np.eye(4), (2, 1, 1)))
    np.testing.assert_allclose(out["T"][2], np.eye(4), rtol=0, atol=1e-9)       # a fragment onto itself


# --------------------------------------------------------------------------------------------------------------- CLI
def test_pairwise_demo_fpfh_needs_no_checkpoint(gpu, tmp_path, monkeypatch, capsys):
    """scripts/pairwise_demo.py --fpfh --icp on the reference's demo pair: no --model, no network; T is printed and
    written to est_T.log.  The pair has no ground truth here: its fitness is printed, not asserted."""
    from lib.utils import read_trajectory, load_config
    from scripts.pairwise_demo import main, parser
    src, tgt = os.path.join(DEMO, "cloud_bin_0.ply"), os.path.join(DEMO, "cloud_bin_1.ply")
    monkeypatch.chdir(tmp_path)
    assert not os.path.exists("pretrained")
    for extra in ([], ["--icp", "--fpfh_radius", "0.1", "--normal_radius", "0.06"]):
        a = parser().parse_args([DEMO_CFG, "--source_pc", src, "--target_pc", tgt, "--fpfh"] + extra)
        T = main(load_config(a.config), a)
        printed = capsys.readouterr().out
        assert "T (source -> target)" in printed
        rows = [ln.replace("[", " ").replace("]", " ").split() for ln in printed.splitlines()[-4:]]
        np.testing.assert_allclose(np.asarray(rows, dtype=np.float64), T, rtol=0, atol=1e-7)
        assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-9 and (T[3] == [0.0, 0.0, 0.0, 1.0]).all()
        keys, traj = read_trajectory(str(tmp_path / "data/demo/pairwise/results/est_T.log"))
        assert keys.tolist() == [["0", "1", "True"]]
        np.testing.assert_allclose(traj[0], T, atol=1e-9)
