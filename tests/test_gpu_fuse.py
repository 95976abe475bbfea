"""GPU scene fusion (csrc/fuse.hip mvr_fuse_scene, lib.multiview.fuse_scene / register_scene, scripts/fuse_scene.py)
against the numpy oracle (tests/fuse_oracle.py).

Tolerances.  The oracle runs on the GPU's own points and normals and sums in the contract's order, so the voxel set,
n_points and n_frags must match exactly, and xyz / normals differ only by the few ulp a contracted multiply-add moves
a mapped point (inputs below 16 m: about 4e-15 each): atol 1e-12 leaves two orders of margin and sits far below any
indexing error, which is at least a voxel's width.  That no point is close enough to a voxel face for those ulp to
change its voxel is a condition of the cases (fuse_oracle.MARGIN, asserted by test_fuse_host.py and again here on the
GPU's own points).  Under identity poses the transform is exact and xyz must match bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

import fuse_oracle as F
import icp_oracle as O

pytestmark = pytest.mark.gpu
SENTINEL = -77.0


def _split(fo, x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    return [x[fo.off[b]:fo.off[b + 1]] for b in range(fo.B)]


def _raw(dev, frags, R, t, voxel, member=None, normals=None, poses=None):
    """mvr_fuse_scene through the C ABI on sentinel-filled outputs -> (rc, count, dict of the first count rows)"""
    import torch
    from lib import _native as N
    L = N.lib()
    B = len(frags)
    off = np.concatenate([[0], np.cumsum([len(f) for f in frags])]).astype(np.int64)
    M = int(off[-1])
    cat = np.concatenate([np.asarray(f, np.float64).reshape(-1, 3) for f in frags])
    xyz = torch.from_numpy(cat).to(dev)
    nrm = None if normals is None else torch.from_numpy(
        np.concatenate([np.asarray(n, np.float64).reshape(-1, 3) for n in normals])).to(dev)
    if poses is None:
        poses = np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(B, 3, 1)], 2)
    g_poses = torch.from_numpy(np.ascontiguousarray(poses).reshape(B, 12)).to(dev)
    g_off = torch.from_numpy(off).to(dev)
    g_mem = None if member is None else torch.from_numpy(np.asarray(member, np.uint8)).to(dev)
    cap = max(M, 1)
    out_xyz = torch.full((cap, 3), SENTINEL, dtype=torch.float64, device=dev)
    out_nrm = None if nrm is None else torch.full((cap, 3), SENTINEL, dtype=torch.float64, device=dev)
    n_points = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    n_frags = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -99, dtype=torch.int64, device=dev)
    ws_b = L.mvr_fuse_scene_workspace_bytes(M)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
    rc = L.mvr_fuse_scene(N.ptr(xyz) if M else None, N.ptr(nrm) if M else None, N.ptr(g_off), B, M, N.ptr(g_poses),
                          N.ptr(g_mem), float(voxel), N.ptr(ws), ws_b, N.ptr(out_xyz),
                          N.ptr(out_nrm) if M else None, N.ptr(n_points), N.ptr(n_frags), N.ptr(count), N.stream())
    V = int(count.item())
    k = max(V, 0)
    if rc == 0 and V >= 0:   # nothing beyond the count is written (with -1 the rows are not meaningful)
        assert (out_xyz[k:] == SENTINEL).all() and (n_points[k:] == -7).all() and (n_frags[k:] == -7).all()
    return rc, V, {"xyz": out_xyz[:k].cpu().numpy(), "n_points": n_points[:k].cpu().numpy(),
                   "n_frags": n_frags[:k].cpu().numpy(),
                   "normals": None if out_nrm is None else out_nrm[:k].cpu().numpy()}


def _compare(what, got, want, exact):
    """voxel set and counts exactly; xyz / normals bit for bit (exact) or to 1e-12"""
    assert want["margin"] >= F.MARGIN and not want["over_range"], (what, want["margin"])
    assert got["xyz"].shape == want["xyz"].shape, (what, got["xyz"].shape, want["xyz"].shape)
    np.testing.assert_array_equal(got["n_points"], want["n_points"], err_msg=what)
    np.testing.assert_array_equal(got["n_frags"], want["n_frags"], err_msg=what)
    dx = np.abs(got["xyz"] - want["xyz"]).max() if len(want["xyz"]) else 0.0
    dn, short = 0.0, 0
    if want["normals"] is not None:
        ok = want["normal_len"] >= F.SHORT_NORMAL
        short = int((~ok).sum())
        dn = np.abs(got["normals"] - want["normals"])[ok].max() if ok.any() else 0.0
        np.testing.assert_allclose(np.linalg.norm(got["normals"], axis=1), 1.0, rtol=0, atol=1e-12)
    print("%s: %d voxels, margin %.3g; |xyz - oracle| <= %.3g, |normal - oracle| <= %.3g (%d short sums left out)"
          % (what, len(want["xyz"]), want["margin"], dx, dn, short))
    if exact:
        assert got["xyz"].tobytes() == want["xyz"].tobytes(), what
    assert dx <= 1e-12 and dn <= 1e-12, what
    return short


# -------------------------------------------------------------------------------------------------------- the scene
@functools.lru_cache(maxsize=None)
def _scene_fo():
    """the four-fragment scene's 0.025 m centroids with normals oriented to one point of the scene"""
    from lib.overlap import FragmentOverlap
    fo = FragmentOverlap(O.scene4()[0], "FCGF", 0.025)
    fo.estimate_normals(viewpoints=F.scene_viewpoints(O.scene4()[1]))
    return fo


def _scene_poses():
    poses = np.asarray(O.scene4()[1], np.float64)
    return poses[:, :3, :3].copy(), poses[:, :3, 3].copy()


@functools.lru_cache(maxsize=None)
def _scene_oracle(voxel):
    fo = _scene_fo()
    R, t = _scene_poses()
    return F.fuse(_split(fo, fo.xyz), R, t, voxel, normals=_split(fo, fo.normals))


@pytest.mark.parametrize("voxel", [0.025, 0.1])
def test_scene_matches_oracle(gpu, voxel):
    from lib.multiview import fuse_scene
    fo = _scene_fo()
    R, t = _scene_poses()
    want = _scene_oracle(voxel)
    assert (want["normal_len"] < F.SHORT_NORMAL).sum() == 0                      # the cap on this scene: none
    out = fuse_scene(fo, R, t, voxel)
    assert set(out) == {"xyz", "normals", "n_points", "n_frags", "voxel_size"} and out["voxel_size"] == voxel
    assert out["xyz"].device == fo.xyz.device and str(out["xyz"].dtype) == "torch.float64"
    assert str(out["n_points"].dtype) == str(out["n_frags"].dtype) == "torch.int32"
    got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}
    assert _compare("scene4, voxel %g" % voxel, got, want, exact=False) == 0
    assert (want["n_frags"] >= 2).sum() > 100 and got["n_points"].sum() == fo.M
    # determinism: a second call returns the same bytes
    again = fuse_scene(fo, R, t, voxel)
    for k in ("xyz", "normals", "n_points", "n_frags"):
        assert again[k].cpu().numpy().tobytes() == got[k].tobytes(), k
    # normals=False: the same rows without normals
    bare = fuse_scene(fo, R, t, voxel, normals=False)
    assert bare["normals"] is None and bare["xyz"].cpu().numpy().tobytes() == got["xyz"].tobytes()


def test_scene_under_identity_poses_is_bit_exact(gpu):
    fo = _scene_fo()
    frags, nrm = _split(fo, fo.xyz), _split(fo, fo.normals)
    R, t = np.tile(np.eye(3), (4, 1, 1)), np.zeros((4, 3))
    want = F.fuse(frags, R, t, 0.025, normals=nrm)
    rc, V, got = _raw(gpu, frags, R, t, 0.025, normals=nrm)
    assert rc == 0 and V == len(want["xyz"])
    _compare("scene4, identity poses", got, want, exact=True)


def test_filters_keep_the_oracles_rows(gpu):
    from lib.multiview import fuse_scene
    fo = _scene_fo()
    R, t = _scene_poses()
    want = _scene_oracle(0.025)
    full = fuse_scene(fo, R, t, 0.025)
    for kw, keep in ((dict(min_frags=2), want["n_frags"] >= 2), (dict(min_points=3), want["n_points"] >= 3),
                     (dict(min_frags=2, min_points=4), (want["n_frags"] >= 2) & (want["n_points"] >= 4))):
        out = fuse_scene(fo, R, t, 0.025, **kw)
        assert 0 < keep.sum() < len(keep)
        np.testing.assert_array_equal(out["n_frags"].cpu().numpy(), want["n_frags"][keep])
        np.testing.assert_array_equal(out["n_points"].cpu().numpy(), want["n_points"][keep])
        assert out["xyz"].cpu().numpy().tobytes() == full["xyz"].cpu().numpy()[keep].tobytes()
        assert out["normals"].cpu().numpy().tobytes() == full["normals"].cpu().numpy()[keep].tobytes()


# ------------------------------------------------------------------------------------------ small and boundary shapes
def test_run_and_tile_boundaries(gpu):
    """1, 255 .. 4097 points, each in a voxel of its own and all in one voxel (a run of 4097; the sort's tile is 4096),
    under identity poses: bit for bit"""
    for name, (frags, R, t, nrm) in F.size_cases().items():
        want = F.fuse(frags, R, t, F.V_SMALL, normals=nrm)
        rc, V, got = _raw(gpu, frags, R, t, F.V_SMALL, normals=nrm)
        assert rc == 0 and V == len(want["xyz"]), name
        _compare(name, got, want, exact=True)
        n = len(frags[0])
        assert (V == n) if name.startswith("spread") else (V == 1 and got["n_points"][0] == n)


def test_ragged_fragments_member_mask_and_three_fragment_run(gpu):
    frags, R, t, nrm = F.ragged_case()
    assert [len(f) for f in frags] == [0, 300, 0, 1, 700, 300, 0]                # empty first, in the middle, last
    want = F.fuse(frags, R, t, F.V_SMALL, normals=nrm)
    rc, V, got = _raw(gpu, frags, R, t, F.V_SMALL, normals=nrm)
    assert rc == 0 and V == len(want["xyz"])
    _compare("ragged", got, want, exact=False)
    assert (got["n_frags"] >= 2).sum() >= 100
    # a fragment masked out: the call without it, bit for bit (the masked call and the shorter call see the same
    # mapped points in the same order)
    for out_b in (1, 4, 6):
        member = np.ones(7, np.uint8)
        member[out_b] = 0
        keep = [b for b in range(7) if b != out_b]
        rc1, V1, a = _raw(gpu, frags, R, t, F.V_SMALL, member=member, normals=nrm)
        rc2, V2, b = _raw(gpu, [frags[k] for k in keep], R[keep], t[keep], F.V_SMALL, normals=[nrm[k] for k in keep])
        assert rc1 == rc2 == 0 and V1 == V2 > 0
        for k in ("xyz", "normals", "n_points", "n_frags"):
            assert a[k].tobytes() == b[k].tobytes(), (out_b, k)
        _compare("ragged without fragment %d" % out_b, a,
                 F.fuse(frags, R, t, F.V_SMALL, member=member, normals=nrm), exact=False)
    rc, V, _ = _raw(gpu, frags, R, t, F.V_SMALL, member=np.zeros(7, np.uint8))  # no member point
    assert rc == 0 and V == 0
    # a run that spans three fragments, negative coordinates, identity poses
    frags, R, t, nrm = F.three_fragment_run_case()
    want = F.fuse(frags, R, t, F.V_SMALL, normals=nrm)
    rc, V, got = _raw(gpu, frags, R, t, F.V_SMALL, normals=nrm)
    assert rc == 0 and V == 5
    _compare("three-fragment run", got, want, exact=True)
    assert got["n_frags"].max() == 3 and got["n_points"].max() == 5 and (got["xyz"] < 0).all()


def test_empty_scene_range_limit_and_arguments(gpu):
    import torch
    from lib import _native as N
    from lib.multiview import fuse_scene
    from lib.overlap import FragmentOverlap
    L = N.lib()
    # M == 0: count 0, the point arrays and the workspace may be NULL
    count = torch.full((1,), -99, dtype=torch.int64, device=gpu)
    off = torch.zeros(3, dtype=torch.int64, device=gpu)
    assert L.mvr_fuse_scene(None, None, N.ptr(off), 2, 0, None, None, 0.05, None, 0, None, None, None, None,
                            N.ptr(count), N.stream()) == 0
    assert int(count.item()) == 0
    rc, V, got = _raw(gpu, [np.zeros((0, 3))] * 2, np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3)), 0.05)
    assert rc == 0 and V == 0
    # a fragment posed 2^21 voxels away: -1 from the C call, ValueError from Python; two voxels nearer it fits
    frags, R, t = F.far_case()
    assert F.fuse(frags, R, t, F.V_SMALL)["over_range"]
    rc, V, _ = _raw(gpu, frags, R, t, F.V_SMALL)
    assert rc == 0 and V == -1
    fo = FragmentOverlap(frags, "3DMatch", radius=0.1)
    with pytest.raises(ValueError, match="21-bit"):
        fuse_scene(fo, R, t, F.V_SMALL)
    near = t.copy()
    near[1, 1] -= 2 * F.V_SMALL
    want = F.fuse(frags, R, near, F.V_SMALL)
    rc, V, got = _raw(gpu, frags, R, near, F.V_SMALL)
    assert rc == 0 and V == 2 and not want["over_range"]
    np.testing.assert_array_equal(got["n_points"], [5, 5])
    np.testing.assert_allclose(got["xyz"], want["xyz"], rtol=0, atol=1e-9)          # 1e5 m away: ulp 1.5e-11
    assert fuse_scene(fo, R, t, F.V_SMALL, member=[1, 0])["n_points"].tolist() == [5]
    # a NaN pose entry through the C call: -1
    poses = np.concatenate([R, t.reshape(2, 3, 1) * 0.0], 2)
    for at in ((0, 0, 0), (1, 2, 3)):
        bad = poses.copy()
        bad[at] = np.nan
        rc, V, _ = _raw(gpu, frags, None, None, F.V_SMALL, poses=bad)
        assert rc == 0 and V == -1, at
    bad = poses.copy()
    bad[1, 0, 3] = np.inf
    rc, V, _ = _raw(gpu, frags, None, None, F.V_SMALL, poses=bad)
    assert rc == 0 and V == -1
    # MVR_EINVAL, scalars first (NULL pointers everywhere: a scalar is what is rejected)
    z = None
    c = N.ptr(count)
    s = N.stream()
    assert L.mvr_fuse_scene(z, z, z, 2, -1, z, z, 0.05, z, 0, z, z, z, z, c, s) == -1
    assert L.mvr_fuse_scene(z, z, z, 2, 1 << 31, z, z, 0.05, z, 0, z, z, z, z, c, s) == -1
    assert L.mvr_fuse_scene(z, z, z, 0, 0, z, z, 0.05, z, 0, z, z, z, z, c, s) == -1
    assert L.mvr_fuse_scene(z, z, z, 2, 0, z, z, 0.0, z, 0, z, z, z, z, c, s) == -1
    assert L.mvr_fuse_scene(z, z, z, 2, 0, z, z, float("nan"), z, 0, z, z, z, z, c, s) == -1
    assert L.mvr_fuse_scene(z, z, z, 2, 0, z, z, 0.05, z, 0, z, z, z, z, z, s) == -1
    # with points: a missing pointer, a short workspace, exactly one of normals / out_normals
    x = torch.zeros(10, 3, dtype=torch.float64, device=gpu)
    o = torch.zeros(10, dtype=torch.int32, device=gpu)
    off = torch.tensor([0, 10], dtype=torch.int64, device=gpu)
    p = torch.eye(3, 4, dtype=torch.float64, device=gpu).reshape(1, 12).contiguous()
    ws_b = L.mvr_fuse_scene_workspace_bytes(10)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=gpu)
    px, po, pf, pp, pw = N.ptr(x), N.ptr(o), N.ptr(off), N.ptr(p), N.ptr(ws)
    good = [px, z, pf, 1, 10, pp, z, 0.05, pw, ws_b, px, z, po, po, c, s]
    for at in (0, 2, 5, 8, 10, 12, 13):
        args = list(good)
        args[at] = z
        assert L.mvr_fuse_scene(*args) == -1, at
    args = list(good)
    args[9] = ws_b - 1
    assert L.mvr_fuse_scene(*args) == -1
    for at in (1, 11):
        args = list(good)
        args[at] = px
        assert L.mvr_fuse_scene(*args) == -1, at
    assert ctypes.sizeof(ctypes.c_size_t) == 8 and ws_b > 10 * 60


# --------------------------------------------------------------------------------------------------------------- CLI
def test_fuse_scene_cli_writes_the_fused_cloud(gpu, tmp_path):
    from lib.multiview import fuse_scene
    from lib.overlap import FragmentOverlap
    from lib.ply import read_ply_xyz, write_ply_xyz
    from scripts.fuse_scene import main, read_poses
    from scripts.multiview_sync import write_poses
    raw = [f[::8] for f in O.scene4()[0]]
    files = []
    for b, f in enumerate(raw):
        files.append(str(tmp_path / ("frag_%d.ply" % b)))
        write_ply_xyz(files[-1], f)
    write_poses(np.asarray(O.scene4()[1]), str(tmp_path / "poses.txt"))
    poses = read_poses(str(tmp_path / "poses.txt"), 4)                           # rounded to 12 decimals
    base = ["--poses", str(tmp_path / "poses.txt"), "--fragments"] + files + ["--voxel_size", "0.05"]
    main(base + ["--out", str(tmp_path / "out" / "scene.ply")])
    fo = FragmentOverlap(raw, "3DMatch", radius=0.15)
    want = fuse_scene(fo, poses[:, :3, :3], poses[:, :3, 3], 0.05)
    got = read_ply_xyz(str(tmp_path / "out" / "scene.ply"))
    assert len(got) > 100 and got.tobytes() == want["xyz"].cpu().numpy().astype(np.float32).tobytes()
    # --min_frags and --normals: the filtered rows, with the normals after the points
    main(base + ["--min_frags", "2", "--normals", "--normal_radius", "0.1", "--out", str(tmp_path / "two.ply")])
    fo = FragmentOverlap(raw, "3DMatch", radius=0.1)
    fo.estimate_normals(0.1, np.zeros((4, 3)))
    want = fuse_scene(fo, poses[:, :3, :3], poses[:, :3, 3], 0.05, min_frags=2)
    blob = open(str(tmp_path / "two.ply"), "rb").read()
    rows = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], "<f4").reshape(-1, 6)
    assert 0 < len(rows) < len(got) and (want["n_frags"] >= 2).all()
    assert rows[:, :3].tobytes() == want["xyz"].cpu().numpy().astype(np.float32).tobytes()
    assert rows[:, 3:].tobytes() == want["normals"].cpu().numpy().astype(np.float32).tobytes()
    assert read_ply_xyz(str(tmp_path / "two.ply")).tobytes() == rows[:, :3].tobytes()


# ---------------------------------------------------------------------------------------------------- register_scene
def _rot_deg(Ra, Rb):
    return np.rad2deg(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def test_register_scene_with_init_is_the_chain_by_hand(gpu, tmp_path):
    """plumbing, not accuracy: the poses equal, bit for bit, those of the same library calls made here"""
    from lib.icp import icp_refine, information_matrix
    from lib.multiview import fuse_scene, optimize_pose_graph, register_scene, synchronize
    from lib.overlap import FragmentOverlap
    raw = O.scene4()[0]
    init = O.scene4_starts(O.SIX, O.scene4_centroids())
    res = register_scene(raw, 0.025, init=init, method="point_to_plane", min_frags=2)
    pairs = np.asarray(O.SIX)
    fo = FragmentOverlap(raw, "FCGF", 0.025)
    fo.estimate_normals(None, np.zeros((4, 3)))
    overlap = fo.ratios(pairs, np.linalg.inv(init))
    kept = overlap >= 0.3
    ref = icp_refine(fo, pairs[kept], init[kept], method="point_to_plane")
    info = information_matrix(fo, pairs[kept], ref["T"])
    sync = synchronize(ref["T"][:, :3, :3], ref["T"][:, :3, 3], pairs[kept], 4, irls_iters=5)
    pg = optimize_pose_graph(sync["R"], sync["t"], ref["T"][:, :3, :3], ref["T"][:, :3, 3], pairs[kept],
                             info["info"], sync["weights"])
    scene = fuse_scene(fo, pg["R"], pg["t"], 0.025, member=pg["member"], min_frags=2)
    rec = res["pairs"]
    print("register_scene(init): overlap %s, kept %d of 6, fitness %s" % (np.round(overlap, 3), kept.sum(),
                                                                        np.round(rec["fitness"], 3)))
    assert kept.sum() >= 3 and rec["kept"].tolist() == kept.tolist() and rec["overlap"].tobytes() == overlap.tobytes()
    assert rec["pairs"].tolist() == pairs.tolist() and rec["T_coarse"].tobytes() == init.tobytes()
    assert rec["T"][kept].tobytes() == ref["T"].tobytes() and rec["T"][~kept].tobytes() == init[~kept].tobytes()
    assert rec["fitness"][kept].tobytes() == ref["fitness"].tobytes() and not rec["fitness"][~kept].any()
    assert res["R"].tobytes() == pg["R"].tobytes() and res["t"].tobytes() == pg["t"].tobytes()
    assert res["poses"][:, :3, :3].tobytes() == pg["R"].tobytes() and (res["poses"][:, 3] == [0, 0, 0, 1]).all()
    assert res["member"].tolist() == [1, 1, 1, 1]
    for k in ("xyz", "normals", "n_points", "n_frags"):
        assert res["scene"][k].cpu().numpy().tobytes() == scene[k].cpu().numpy().tobytes(), k
    assert (res["scene"]["n_frags"] >= 2).all() and len(res["scene"]["xyz"]) > 100


def test_register_scene_cli_writes_poses_traj_and_scene(gpu, tmp_path, capsys):
    """scripts/register_scene.py on PLY files with --init: poses.txt, traj.txt and scene.ply hold what
    register_scene returns for the same points and estimates (the files to their 12 decimals / float32)"""
    from lib.multiview import register_scene
    from lib.ply import read_ply_xyz, write_ply_xyz
    from lib.utils import read_trajectory, write_trajectory
    from scripts.fuse_scene import read_poses
    from scripts.register_scene import main, read_init
    raw = [f[::2] for f in O.scene4()[0]]
    files = []
    for b, f in enumerate(raw):
        files.append(str(tmp_path / ("frag_%d.ply" % b)))
        write_ply_xyz(files[-1], f)
    start = O.scene4_starts(O.SIX, O.scene4_centroids())
    write_trajectory(np.linalg.inv(start), [[i, j, True] for i, j in O.SIX], str(tmp_path / "init.txt"))
    out = str(tmp_path / "out")
    main(["--fragments"] + files + ["--out", out, "--init", str(tmp_path / "init.txt"), "--min_frags", "2"])
    assert "registered 4 fragments" in capsys.readouterr().out
    want = register_scene([read_ply_xyz(f) for f in files], 0.025, init=read_init(str(tmp_path / "init.txt"), 4),
                          min_frags=2)
    np.testing.assert_allclose(read_poses(out + "/poses.txt", 4), want["poses"], rtol=0, atol=1e-11)
    keys, traj = read_trajectory(out + "/traj.txt")
    kept = want["pairs"]["kept"]
    assert kept.sum() >= 3 and [[int(k[0]), int(k[1])] for k in keys] == want["pairs"]["pairs"][kept].tolist()
    np.testing.assert_allclose(traj, np.linalg.inv(want["pairs"]["T"][kept]), rtol=0, atol=1e-11)
    blob = open(out + "/scene.ply", "rb").read()
    rows = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], "<f4").reshape(-1, 6)
    assert len(rows) > 100 and rows[:, :3].tobytes() == want["scene"]["xyz"].cpu().numpy().astype("<f4").tobytes()
    assert rows[:, 3:].tobytes() == want["scene"]["normals"].cpu().numpy().astype("<f4").tobytes()


def test_register_scene_weights_free(gpu, tmp_path):
    """fragment 0's centroids and two moved copies of them with distractors (icp_oracle.full_copy_case, the
    construction of test_gpu_fpfh.py, viewpoints moved along): FPFH + RANSAC, the gate, ICP, synchronisation,
    refinement and fusion in one call.  Every pose must land within the bound test_gpu_fpfh.py imposes on the coarse
    stage for this construction: RANSAC_DIST at the fragment's centroid and 1 degree.  The refined error is printed:
    near 1e-9 is expected where fragment 0 is the source; the copy-to-copy pair carries both copies' distractors."""
    from lib.multiview import register_scene
    from lib.utils import RANSAC_DIST
    src = O.scene4_centroids()[0]
    c = src.mean(0)
    copies = [O.full_copy_case(src, seed=s) for s in (3, 5)]
    frags = [src] + [cp[0] for cp in copies]
    truth = [np.eye(4)] + [np.linalg.inv(cp[1]) for cp in copies]            # fragment -> fragment 0's frame
    views = np.asarray([c] + [cp[1][:3, :3] @ c + cp[1][:3, 3] for cp in copies])
    res = register_scene(frags, 0.025, viewpoints=views, downsample=False, seed=0)
    rec = res["pairs"]
    print("register_scene: overlap %s kept %s fitness %s rmse %s" % (np.round(rec["overlap"], 3), rec["kept"],
                                                                   np.round(rec["fitness"], 4), rec["rmse"]))
    assert res["member"].tolist() == [1, 1, 1] and rec["kept"][:2].all()
    for k, cp in enumerate(copies):                                              # pairs (0, 1) and (0, 2)
        print("pair (0, %d) after ICP: |T - T_true| %.3g" % (k + 1, np.abs(rec["T"][k] - cp[1]).max()))
    for b in range(3):
        cb = views[b]                                                            # the fragment's centroid, own frame
        M, G = res["poses"][b], truth[b]
        dt = np.linalg.norm((M[:3, :3] @ cb + M[:3, 3]) - (G[:3, :3] @ cb + G[:3, 3]))
        dr = _rot_deg(M[:3, :3], G[:3, :3])
        print("fragment %d: off by %.3g m at its centroid, %.3g deg; |pose - truth| %.3g"
              % (b, dt, dr, np.abs(M - G).max()))
        assert dt <= RANSAC_DIST and dr <= 1.0
    scene = res["scene"]
    nf = scene["n_frags"].cpu().numpy()
    print("fused: %d voxels, %d seen by all three fragments" % (len(nf), int((nf == 3).sum())))
    assert (nf == 3).sum() > 0 and scene["normals"] is not None and scene["n_points"].sum().item() == sum(
        len(f) for f in frags)
