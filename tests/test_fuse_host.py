"""Host-side checks of scene fusion: the numpy oracle (tests/fuse_oracle.py) against the independent dict version
of VoxelDownSample and against cases worked by hand, the face margin of every case the GPU test compares, the PLY
writer, and the argument checks of lib.multiview.fuse_scene / register_scene and of the two scripts' parsers."""
import types

import numpy as np
import pytest

import fuse_oracle as F
import icp_oracle as O
from overlap_cases import lexsorted, voxel_down_sample_dict

I3 = np.eye(3)


def test_identity_pose_one_fragment_equals_the_dict_version():
    rng = np.random.default_rng(0)
    for n, v in ((1, 0.05), (500, 0.05), (2000, 0.11)):
        p = rng.uniform(-1.0, 1.0, (n, 3))
        got = F.fuse([p], I3[None], np.zeros((1, 3)), v)
        want = voxel_down_sample_dict(p, v)
        assert lexsorted(got["xyz"]).tobytes() == lexsorted(want).tobytes()
        assert got["n_points"].sum() == n and (got["n_frags"] == 1).all() and not got["over_range"]
        assert (np.diff(got["keys"].astype(np.int64)) > 0).all()


def test_two_fragments_in_one_voxel():
    a, b = np.array([[0.25, 0.5, 0.5]]), np.array([[0.5, 0.25, 0.25]])
    got = F.fuse([a, b], np.tile(I3, (2, 1, 1)), np.zeros((2, 3)), 1.0)
    # lo = (0.25, 0.25, 0.25) - 0.5: both indices are (0, 0, 0)
    assert got["n_points"].tolist() == [2] and got["n_frags"].tolist() == [2] and got["keys"].tolist() == [0]
    np.testing.assert_array_equal(got["xyz"], [[0.375, 0.375, 0.375]])
    # two points of one fragment: one fragment
    one = F.fuse([np.concatenate([a, b])], I3[None], np.zeros((1, 3)), 1.0)
    assert one["n_points"].tolist() == [2] and one["n_frags"].tolist() == [1]
    # a pose that moves b a voxel along z: two voxels, keys 0 and 1
    apart = F.fuse([a, b], np.tile(I3, (2, 1, 1)), np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.5]]), 1.0)
    assert apart["keys"].tolist() == [0, 1] and apart["n_frags"].tolist() == [1, 1]
    np.testing.assert_array_equal(apart["xyz"], [[0.25, 0.5, 0.5], [0.5, 0.25, 1.75]])


def test_opposite_normals_give_the_z_axis():
    p = [np.array([[0.25, 0.5, 0.5]]), np.array([[0.5, 0.25, 0.25]])]
    n = [np.array([[0.0, 1.0, 0.0]]), np.array([[0.0, -1.0, 0.0]])]
    got = F.fuse(p, np.tile(I3, (2, 1, 1)), np.zeros((2, 3)), 1.0, normals=n)
    np.testing.assert_array_equal(got["normals"], [[0.0, 0.0, 1.0]])
    assert got["normal_len"].tolist() == [0.0]
    # the rotation applies to the normals, the translation does not: Rz(90 deg) takes +y to -x
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    got = F.fuse(p[:1], Rz[None], np.array([[5.0, 5.0, 5.0]]), 1.0, normals=n[:1])
    np.testing.assert_array_equal(got["normals"], [[-1.0, 0.0, 0.0]])
    np.testing.assert_array_equal(got["xyz"], [[4.5, 5.25, 5.5]])


def test_negative_coordinates_and_the_three_fragment_run():
    got = F.fuse([np.array([[-1.25, -0.5, -3.0], [-0.75, -0.5, -3.0]])], I3[None], np.zeros((1, 3)), 1.0)
    # lo = (-1.75, -1.0, -3.5): indices (0, 0, 0) and (1, 0, 0)
    assert got["keys"].tolist() == [0, 1 << 42]
    np.testing.assert_array_equal(got["xyz"], [[-1.25, -0.5, -3.0], [-0.75, -0.5, -3.0]])
    frags, R, t, nrm = F.three_fragment_run_case()
    got = F.fuse(frags, R, t, F.V_SMALL, normals=nrm)
    at = got["keys"].tolist().index((4 << 42) | (4 << 21) | 4)
    assert got["n_points"][at] == 5 and got["n_frags"][at] == 3 and got["n_points"].sum() == 9
    assert sorted(got["n_points"].tolist()) == [1, 1, 1, 1, 5] and (got["xyz"] < 0).all()
    rows = np.concatenate([frags[0][:2], frags[1][:1], frags[3][:2]])
    np.testing.assert_allclose(got["xyz"][at], rows.mean(0), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(got["normals"], np.tile([0.0, 0.0, 1.0], (5, 1)))


def test_member_and_range():
    frags, R, t, nrm = F.three_fragment_run_case()
    masked = F.fuse(frags, R, t, F.V_SMALL, member=[1, 1, 0, 1], normals=nrm)
    without = F.fuse([frags[0], frags[1], frags[3]], R[[0, 1, 3]], t[[0, 1, 3]], F.V_SMALL,
                     normals=[nrm[0], nrm[1], nrm[3]])
    assert masked["xyz"].tobytes() == without["xyz"].tobytes() and masked["n_frags"].tolist() == [1, 1, 3, 1]
    assert F.fuse(frags, R, t, F.V_SMALL, member=[0, 0, 0, 0])["xyz"].shape == (0, 3)
    far, Rf, tf = F.far_case()
    assert F.fuse(far, Rf, tf, F.V_SMALL)["over_range"]
    tf = tf.copy()
    tf[1, 1] -= 2 * F.V_SMALL       # two voxels nearer: the last index is 2^21 - 1 or - 2
    near = F.fuse(far, Rf, tf, F.V_SMALL)
    assert not near["over_range"] and near["n_points"].tolist() == [5, 5]
    Rn = Rf.copy()
    Rn[0, 1, 1] = np.nan
    assert F.fuse(far, Rn, tf, F.V_SMALL)["over_range"]


def _cases():
    out = dict(F.size_cases())
    out["ragged"] = F.ragged_case()
    out["three_fragment_run"] = F.three_fragment_run_case()
    return out


def test_every_gpu_case_keeps_its_points_off_the_voxel_faces():
    """a condition of test_gpu_fuse.py: a contracted multiply-add moves a mapped point by a few ulp, which changes its
    voxel only within about 1e-12 of a face"""
    for name, (frags, R, t, nrm) in _cases().items():
        got = F.fuse(frags, R, t, F.V_SMALL, normals=nrm)
        n = sum(len(f) for f in frags)
        assert got["margin"] >= F.MARGIN and not got["over_range"], (name, got["margin"])
        assert got["n_points"].sum() == n
        if name.startswith("spread"):
            assert len(got["xyz"]) == n and (got["n_points"] == 1).all(), name
        if name.startswith("clump"):
            assert got["n_points"].tolist() == [n], name
    rag = F.fuse(*F.ragged_case()[:3], F.V_SMALL)
    assert (rag["n_frags"] >= 2).sum() >= 100 and rag["n_frags"].max() <= 3      # fragments 1 and 5 share voxels


def test_scene_cases_keep_the_margin_and_have_no_short_normal():
    """the four-fragment scene under its ground-truth poses at both voxel sizes, on the host's centroids (the GPU's
    are the same point sets in another order, test_gpu_overlap.py) and the host's normals over the GPU test's radius
    (icp_plane_oracle), oriented as the GPU test orients them: no voxel's summed normal is shorter than
    SHORT_NORMAL, so the GPU test leaves none out"""
    import icp_plane_oracle as PO
    cent = O.scene4_centroids()
    poses = np.asarray(O.scene4()[1])
    nrm = [d["normals"] for d in PO.estimate_normals_batch(cent, 3 * 0.025, F.scene_viewpoints(poses))]
    for voxel in (0.025, 0.1):
        got = F.fuse(cent, poses[:, :3, :3], poses[:, :3, 3], voxel, normals=nrm)
        print("scene4, voxel %g: %d points -> %d voxels, margin %.3g, %d seen by >= 2 fragments, shortest summed "
              "normal %.3g" % (voxel, got["n_points"].sum(), len(got["xyz"]), got["margin"],
                               int((got["n_frags"] >= 2).sum()), got["normal_len"].min()))
        assert got["margin"] >= F.MARGIN and not got["over_range"]
        assert (got["n_frags"] >= 2).sum() > 100
        assert (got["normal_len"] < F.SHORT_NORMAL).sum() == 0


# ------------------------------------------------------------------------------------------------------------- PLY
def _header_and_body(path):
    raw = open(path, "rb").read()
    at = raw.index(b"end_header\n") + len(b"end_header\n")
    return raw[:at].decode().split("\n")[:-1], raw[at:]


def test_write_ply_round_trip(tmp_path):
    from lib.ply import read_ply_xyz, write_ply, write_ply_xyz
    rng = np.random.default_rng(1)
    xyz, nrm = rng.normal(0, 3, (37, 3)), rng.normal(0, 1, (37, 3))
    a, b, c = (str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply"))
    write_ply(a, xyz)
    write_ply_xyz(b, xyz)
    assert open(a, "rb").read() == open(b, "rb").read()                      # without normals: the bare writer's file
    write_ply(c, xyz, nrm)
    head, body = _header_and_body(c)
    assert head == ["ply", "format binary_little_endian 1.0", "element vertex 37"] + \
        ["property float %s" % n for n in ("x", "y", "z", "nx", "ny", "nz")] + ["end_header"]
    rows = np.frombuffer(body, "<f4").reshape(37, 6)
    assert rows[:, :3].tobytes() == xyz.astype("<f4").tobytes() and rows[:, 3:].tobytes() == nrm.astype("<f4").tobytes()
    for f in (a, c):
        assert read_ply_xyz(f).tobytes() == xyz.astype(np.float32).tobytes()
    write_ply(a, np.zeros((0, 3)), np.zeros((0, 3)))
    assert read_ply_xyz(a).shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(a, xyz, nrm[:5])


# ------------------------------------------------------------------------------------------------------- arguments
def test_fuse_scene_rejects_bad_arguments():
    """every check comes before the device is asked for, so it runs without one"""
    from lib.multiview import fuse_scene
    fo = types.SimpleNamespace(B=2, M=0, normals=None)
    R, t = np.tile(I3, (2, 1, 1)), np.zeros((2, 3))
    bad = [dict(R=R[:1]), dict(R=R.reshape(2, 9)), dict(t=np.zeros((2, 4))), dict(t=np.zeros(3)),
           dict(R=np.where(I3 > 0, np.nan, R)), dict(t=np.full((2, 3), np.inf)), dict(R=R.astype(np.int64)),
           dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")),
           dict(member=[1]), dict(member=[1.0, 0.0]), dict(member=[[1, 1]]), dict(min_frags=0), dict(min_points=0),
           dict(normals=np.zeros((0, 3)))]
    for kw in bad:
        args = dict(R=R, t=t, voxel_size=0.05)
        args.update(kw)
        with pytest.raises(ValueError):
            fuse_scene(fo, **args)


def test_register_scene_rejects_bad_arguments():
    from lib.multiview import register_scene
    pts = [np.zeros((4, 3))] * 3
    bad = [dict(xyz_list=pts[:1]), dict(voxel_size=0.0), dict(method="point_to_line"), dict(dataset="kitti"),
           dict(init=np.tile(np.eye(4), (2, 1, 1))), dict(init=np.full((3, 4, 4), np.nan)),
           dict(viewpoints=np.zeros((2, 3))), dict(xyz_list=[pts[0]] * 129)]
    for kw in bad:
        args = dict(xyz_list=pts)
        args.update(kw)
        with pytest.raises(ValueError):
            register_scene(**args)


def test_fuse_scene_cli_arguments(tmp_path, capsys):
    from scripts.fuse_scene import check_args, parser, read_poses
    from scripts.multiview_sync import write_poses
    ap = parser()
    base = ["--poses", "p.txt", "--fragments", "a.ply", "b.ply", "--voxel_size", "0.05", "--out", "s.ply"]
    a = check_args(ap, ap.parse_args(base))
    assert a.fragments == ["a.ply", "b.ply"] and a.voxel_size == 0.05 and a.min_frags == 1 and not a.normals
    a = check_args(ap, ap.parse_args(base + ["--min_frags", "2", "--normals", "--normal_radius", "0.1"]))
    assert a.min_frags == 2 and a.normals and a.normal_radius == 0.1
    for argv in (base[:-2], base[2:], base + ["--min_frags", "0"], base + ["--normal_radius", "0.1"],
                 base + ["--normals", "--normal_radius", "-1"], base[:6] + ["0", "--out", "s.ply"]):
        with pytest.raises(SystemExit):
            check_args(ap, ap.parse_args(argv))
    capsys.readouterr()
    poses = np.tile(np.eye(4), (3, 1, 1))
    poses[:, :3, 3] = np.arange(9).reshape(3, 3) / 8.0
    write_poses(poses, str(tmp_path / "poses.txt"))
    np.testing.assert_array_equal(read_poses(str(tmp_path / "poses.txt"), 3), poses)
    with pytest.raises(ValueError):
        read_poses(str(tmp_path / "poses.txt"), 2)


def test_register_scene_cli_arguments(tmp_path, capsys):
    from lib import multiview
    from lib.utils import write_trajectory
    from scripts import register_scene as S
    assert S.ICP_METHODS == multiview.ICP_METHODS and set(S.DATASETS) == set(multiview.OVERLAP_THRESHOLDS)
    ap = S.parser()
    base = ["--fragments", "a.ply", "b.ply", "c.ply", "--out", "dir"]
    a = S.check_args(ap, ap.parse_args(base))
    assert (a.voxel_size, a.icp_method, a.init, a.dataset, a.min_frags, a.anchor, a.seed) == \
        (0.025, "point_to_point", None, "3d_match", 1, 0, 0)
    a = S.check_args(ap, ap.parse_args(base + ["--icp_method", "generalized", "--dataset", "redwood", "--anchor", "2"]))
    assert a.icp_method == "generalized" and a.dataset == "redwood" and a.anchor == 2
    for argv in (base[:2] + base[4:], base[:4], base + ["--icp_method", "x"], base + ["--voxel_size", "0"],
                 base + ["--anchor", "3"], base + ["--min_frags", "0"], base + ["--dataset", "kitti"]):
        with pytest.raises(SystemExit):
            S.check_args(ap, ap.parse_args(argv))
    capsys.readouterr()
    # --init: a trajectory in the log convention (inv(T)), any order, every pair i < j
    T = np.asarray([O.rigid([1, 2, 3], 10.0 * (k + 1), [k, 0.5, -k]) for k in range(3)])
    meta = [[1, 2, True], [0, 1, True], [0, 2, True]]
    write_trajectory(np.linalg.inv(T), meta, str(tmp_path / "traj.txt"))
    got = S.read_init(str(tmp_path / "traj.txt"), 3)
    np.testing.assert_allclose(got, T[[1, 2, 0]], rtol=0, atol=1e-9)
    with pytest.raises(ValueError):
        S.read_init(str(tmp_path / "traj.txt"), 4)
