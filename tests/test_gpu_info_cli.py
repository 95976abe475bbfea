"""The command-line surface of the information matrices and the pose-graph refinement, on the synthetic scene of the
harness tests (tests/helpers/eval_layout.py): scripts/benchmark_pairwise_registration.py --write_info and
scripts/multiview_sync.py --info FILE --refine.  Without the flags both scripts write what they wrote before: the
tests run them both ways and compare the files byte for byte."""
import os
import shutil
import sys

import numpy as np
import pytest

import posegraph_oracle as PO

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
if HELPERS not in sys.path:
    sys.path.insert(0, HELPERS)

pytestmark = pytest.mark.gpu
ARGV = ["--method", "RANSAC", "--batch_size", "4", "--num_workers", "0"]


def _scene_dir(root):
    return os.path.join(root, "3d_match", "results", "RANSAC", "all", "kitchen")


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """the benchmark on one scene of 5 fragments: plain, and with --write_info"""
    from eval_layout import write_scene
    from scripts.benchmark_pairwise_registration import main
    base = tmp_path_factory.mktemp("info_cli")
    roots = [str(base / n) for n in ("plain", "info")]
    pairs = write_scene(os.path.join(roots[0], "3d_match"), "kitchen", 5, 600, seed=0)
    shutil.copytree(roots[0], roots[1])
    s0 = main(["--source_path", roots[0]] + ARGV)
    s1 = main(["--source_path", roots[1]] + ARGV + ["--write_info"])
    return roots, pairs, s0, s1


def test_write_info_writes_est_info_beside_traj(gpu, runs):
    from lib.icp import information_matrix
    from lib.overlap import FragmentOverlap
    from lib.utils import read_trajectory, read_trajectory_info
    roots, pairs, s0, s1 = runs
    assert s0 == s1
    assert sorted(os.listdir(_scene_dir(roots[0]))) == ["traj.txt"]                  # no flag: nothing new
    assert sorted(os.listdir(_scene_dir(roots[1]))) == ["est.info", "traj.txt"]
    t0, t1 = (open(os.path.join(_scene_dir(r), "traj.txt"), "rb").read() for r in roots)
    assert t0 == t1 and len(t0) > 0                                                  # and the trajectory is unchanged
    keys, traj = read_trajectory(os.path.join(_scene_dir(roots[1]), "traj.txt"))
    n_frames, info = read_trajectory_info(os.path.join(_scene_dir(roots[1]), "est.info"))
    heads = [ln.split() for ln in open(os.path.join(_scene_dir(roots[1]), "est.info")).read().splitlines()[::7]]
    assert [h[:2] for h in heads] == keys[:, :2].tolist() == [[str(i), str(j)] for i, j in pairs]
    assert info.shape == (len(pairs), 6, 6) and n_frames == 5
    # the matrices are those of the written estimates on the gate's points; info[0, 0] is the correspondence count
    clouds = [np.load(os.path.join(roots[1], "3d_match", "features", "kitchen", "kitchen_%03d.npz" % k))["xyz"]
              for k in range(5)]
    fo = FragmentOverlap(clouds, "FCGF")
    want = information_matrix(fo, pairs, np.linalg.inv(traj))
    print("n_corr %s; |info file - information_matrix(inv(traj))| %.3g of %.3g"
          % (want["n_corr"].tolist(), np.abs(info - want["info"]).max(), np.abs(want["info"]).max()))
    np.testing.assert_array_equal(info[:, 0, 0], want["n_corr"])
    assert want["n_corr"].min() > 100
    # traj.txt holds 12 decimals of the estimate: the re-evaluation starts 1e-12 off, which moves no correspondence
    # on this scene (the fragments are exact copies) and the sums by as much
    np.testing.assert_allclose(info, want["info"], rtol=1e-9, atol=1e-9 * np.abs(want["info"]).max())
    np.testing.assert_array_equal(info, np.transpose(info, (0, 2, 1)))


def test_multiview_sync_refine(gpu, runs, tmp_path, capsys):
    from lib.multiview import synchronize
    from lib.utils import read_trajectory, read_trajectory_info
    from scripts import multiview_sync as MS
    roots, pairs, _, _ = runs
    traj_file = os.path.join(_scene_dir(roots[1]), "traj.txt")
    info_file = os.path.join(_scene_dir(roots[1]), "est.info")
    outs = [str(tmp_path / n) for n in ("plain", "refined", "zero_trials")]
    head = ["--traj", traj_file, "--n_fragments", "5", "--irls", "3"]
    MS.main(head + ["--out", outs[0]])
    assert "refined" not in capsys.readouterr().out
    MS.main(head + ["--out", outs[1], "--info", info_file, "--refine"])
    said = capsys.readouterr().out
    assert "refined over SE(3): cost" in said
    MS.main(head + ["--out", outs[2], "--info", info_file, "--refine", "--refine_iters", "0"])
    with pytest.raises(SystemExit):
        MS.main(head + ["--out", outs[2], "--refine"])
    for name in ("poses.txt", "traj_sync.txt"):        # zero trials: the flags' path adds nothing of its own
        assert open(os.path.join(outs[0], name), "rb").read() == open(os.path.join(outs[2], name), "rb").read(), name
        assert sorted(os.listdir(outs[0])) == sorted(os.listdir(outs[1])) == ["poses.txt", "traj_sync.txt"]
    keys, traj = read_trajectory(traj_file)
    info = read_trajectory_info(info_file)[1]
    T = np.linalg.inv(traj)
    ij = np.asarray(pairs)
    w = synchronize(T[:, :3, :3], T[:, :3, 3], ij, 5, irls_iters=3)["weights"]
    cost = []
    for o in outs[:2]:
        k, poses = read_trajectory(os.path.join(o, "poses.txt"))
        assert poses.shape == (5, 4, 4) and [list(x) for x in k] == [[str(i), str(i), "5"] for i in range(5)]
        cost.append(PO.cost(poses[:, :3, :3], poses[:, :3, 3], T[:, :3, :3], T[:, :3, 3], ij, w, info))
        k2, ts = read_trajectory(os.path.join(o, "traj_sync.txt"))
        assert np.array_equal(k2, keys)
        from lib.multiview import pairwise_from_poses
        np.testing.assert_allclose(ts, np.linalg.inv(pairwise_from_poses(poses[:, :3, :3], poses[:, :3, 3], ij)),
                                   rtol=0, atol=1e-10)
    print("pose-graph cost of poses.txt: synchronised %.6g, refined %.6g; the script said: %s"
          % (cost[0], cost[1], said.strip().splitlines()[-1]))
    assert cost[1] <= cost[0]
