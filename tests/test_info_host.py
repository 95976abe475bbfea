"""Host-side checks of the information matrix (tests/info_oracle.py, lib.icp.permute_information,
lib.utils.write_trajectory_info, the argument rules of mvr_pair_information): the oracle's identities, the file round
trip, what computeTransformationErr makes of the matrix, and that no case test_gpu_info.py uses has a correspondence
decided by rounding.  No GPU."""
import numpy as np
import pytest

import icp_oracle as O
import info_oracle as IO


def _small():
    frags, pairs, T0 = O.small_case()
    return frags, pairs, T0, IO.information_batch(frags, pairs, T0, O.SMALL_MAX_DIST)


def test_oracle_identities():
    frags, pairs, T0, res = _small()
    sizes = [len(frags[s]) for s, _ in pairs]
    assert sizes == list(O.SMALL_SIZES) + [40]
    for n_src, r in zip(sizes, res):
        L, n = r["info"], r["n_corr"]
        assert n <= n_src
        np.testing.assert_array_equal(L, L.T)                               # products commute: exactly symmetric
        np.testing.assert_array_equal(L[:3, :3], n * np.eye(3))
        np.testing.assert_array_equal(L[:3, 3:], -L[3:, :3])                # -[sum y]x and its transpose
        if n >= 3:                                                          # three points off a line: definite
            assert np.linalg.eigvalsh(L).min() > 0.0
        if n == 0:
            assert not L.any() and r["rmse"] == 0.0
    assert [r["n_corr"] for r in res][:4] == [0, 1, 2, 3] and res[-1]["n_corr"] == 0


def test_moment_form_equals_the_literal_sum():
    """what the kernel assembles: [n I, -[sum y]x; [sum y]x, tr(S) I - S] with S = sum y y^T"""
    ys = np.random.default_rng(0).uniform(-2, 3, (57, 3))
    S, m = ys.T @ ys, ys.sum(0)
    want = np.zeros((6, 6))
    want[:3, :3] = len(ys) * np.eye(3)
    want[:3, 3:] = -IO.skew(m)
    want[3:, :3] = IO.skew(m)
    want[3:, 3:] = np.trace(S) * np.eye(3) - S
    np.testing.assert_allclose(IO.information_from_points(ys), want, rtol=0, atol=1e-12 * np.abs(want).max())


def test_quadratic_form_is_the_summed_squared_displacement():
    frags, pairs, T0, res = _small()
    rng = np.random.default_rng(1)
    for r in res:
        v, w = rng.normal(0, 0.01, 3), rng.normal(0, 0.02, 3)
        xi = np.concatenate([v, w])
        direct = np.sum((v + np.cross(w, r["ys"])) ** 2)
        assert abs(xi @ r["info"] @ xi - direct) <= 1e-13 * max(direct, 1e-300) + 1e-30


def test_open3d_permutation_is_an_involution():
    import torch
    from lib.icp import permute_information
    L = np.random.default_rng(2).standard_normal((5, 6, 6))
    P = permute_information(L, "open3d")
    np.testing.assert_array_equal(P, IO.to_open3d(L))
    np.testing.assert_array_equal(P[:, :3, :3], L[:, 3:, 3:])
    np.testing.assert_array_equal(P[:, :3, 3:], L[:, 3:, :3])
    np.testing.assert_array_equal(permute_information(P, "open3d"), L)
    assert permute_information(L, "redwood") is L
    np.testing.assert_array_equal(permute_information(torch.from_numpy(L), "open3d").numpy(), P)
    with pytest.raises(ValueError):
        permute_information(L, "colmap")


def test_write_read_trajectory_info_round_trip(tmp_path):
    from lib.utils import read_trajectory, read_trajectory_info, write_trajectory, write_trajectory_info
    rng = np.random.default_rng(3)
    info = np.stack([IO.information_from_points(rng.uniform(-3, 3, (n, 3))) for n in (4, 900, 17, 60)])
    traj = np.tile(np.eye(4), (4, 1, 1))
    meta = [["0", "1", True], ["0", "2", False], ["1", "2", "True"], ["2", "5", True]]
    write_trajectory_info(info, meta, str(tmp_path / "est.info"))
    write_trajectory(traj, meta, str(tmp_path / "traj.txt"))
    n_frames, got = read_trajectory_info(str(tmp_path / "est.info"))
    keys, _ = read_trajectory(str(tmp_path / "traj.txt"))
    assert n_frames == 6 and got.shape == (3, 6, 6)                         # the record with flag False is skipped
    # the written 12 decimals: half a unit of the last one, and half an ulp of the value where the text is read back
    np.testing.assert_allclose(got, info[[0, 2, 3]], rtol=1.2e-16, atol=0.5e-12)
    heads = [ln.split() for ln in open(str(tmp_path / "est.info")).read().splitlines()[::7]]
    assert [h[:2] for h in heads] == keys[:, :2].tolist() == [["0", "1"], ["1", "2"], ["2", "5"]]
    write_trajectory_info(info, meta, str(tmp_path / "n.info"), n_frames=57)
    assert read_trajectory_info(str(tmp_path / "n.info"))[0] == 57
    write_trajectory_info(info[:0], [], str(tmp_path / "empty.info"))
    assert read_trajectory_info(str(tmp_path / "empty.info"))[1].shape == (0, 6, 6)


def test_transformation_error_is_the_mean_squared_displacement():
    """computeTransformationErr's e = (t, q_xyz): e^T info e / info[0,0] is exactly the mean of |t + q_xyz x y|^2
    over the correspondences.  q_xyz = sin(theta / 2) axis is half the rotation vector to first order, so against the
    true displacement of the points the rotation's share counts a quarter (the factor DESIGN.md 4.22 leaves
    unpinned for Redwood's files); for a pure translation it is the mean squared displacement itself."""
    from lib.utils import computeTransformationErr
    frags, pairs, T0, res = _small()
    r = res[-2]                                                             # the 1025-point source
    assert r["n_corr"] > 500
    M = O.rigid([0.3, -1.0, 0.5], 0.4, [0.004, -0.002, 0.003])
    axis = np.array([0.3, -1.0, 0.5]) / np.linalg.norm([0.3, -1.0, 0.5])
    qv = np.sin(np.deg2rad(0.4) / 2) * axis
    want = np.mean(np.sum((M[:3, 3] + np.cross(qv, r["ys"])) ** 2, 1))
    got = computeTransformationErr(M, r["info"])
    assert abs(got - want) <= 1e-9 * want
    Tt = np.eye(4)
    Tt[:3, 3] = [0.01, 0.02, -0.005]
    moved = r["ys"] + Tt[:3, 3]
    assert abs(computeTransformationErr(Tt, r["info"]) - np.mean(np.sum((moved - r["ys"]) ** 2, 1))) <= 1e-15
    # first order in the angle: the displacement under the rotation by 2 q_xyz (= theta to first order)
    full = O.rigid(axis, 0.4, M[:3, 3])
    disp = np.mean(np.sum((r["ys"] @ full[:3, :3].T + full[:3, 3] - r["ys"]) ** 2, 1))
    half = np.mean(np.sum((M[:3, 3] + np.cross(2 * qv, r["ys"])) ** 2, 1))
    assert abs(disp - half) <= 2e-2 * disp


def test_no_gpu_case_is_decided_by_rounding():
    """every case of test_gpu_info.py: the nearest neighbour and the max_dist test clear rounding by 1e-8"""
    for name, frags, pairs, T, max_dist in IO.cases():
        res = IO.information_batch(frags, pairs, T, max_dist)
        gap = min(r["gap"] for r in res)
        edge = min(r["edge"] for r in res)
        print("%s: gap %.3g, edge %.3g, n_corr %s" % (name, gap, edge, [r["n_corr"] for r in res][:14]))
        assert gap >= 1e-8 and edge >= 1e-8, name


def test_abi_argument_rules_without_a_device():
    from lib import _native as N
    L = N.lib()
    Z = None
    assert L.mvr_pair_information(Z, 0, Z, Z, 2, 0, 0.05, Z, Z, 0, 0.05, Z, Z, Z, Z, Z) == 0      # P = 0, NULLs
    assert L.mvr_pair_information(Z, 0, Z, Z, 2, 0, 0.05, Z, Z, 0, 0.0500001, Z, Z, Z, Z, Z) == -1  # max_dist > r
    assert L.mvr_pair_information(Z, 0, Z, Z, 2, 0, 0.05, Z, Z, 0, 0.0, Z, Z, Z, Z, Z) == -1
    assert L.mvr_pair_information(Z, 0, Z, Z, 0, 0, 0.05, Z, Z, 0, 0.05, Z, Z, Z, Z, Z) == -1     # B <= 0
    assert L.mvr_pair_information(Z, 0, Z, Z, 2, 0, 0.05, Z, Z, -1, 0.05, Z, Z, Z, Z, Z) == -1
    assert L.mvr_pair_information(Z, 0, Z, Z, 2, 0, 0.05, Z, Z, 3, 0.05, Z, Z, Z, Z, Z) == -1     # P > 0, NULLs


def test_wrapper_argument_rules_without_a_device():
    from lib.icp import information_matrix

    class Fo:      # the checks come before anything touches the index
        r = 0.05
    T = np.tile(np.eye(4), (2, 1, 1))
    with pytest.raises(ValueError, match="exceeds"):
        information_matrix(Fo, [[0, 1], [1, 0]], T, max_dist=0.06)
    with pytest.raises(ValueError, match="positive"):
        information_matrix(Fo, [[0, 1], [1, 0]], T, max_dist=0.0)
    with pytest.raises(ValueError, match="order"):
        information_matrix(Fo, [[0, 1], [1, 0]], T, order="colmap")
    with pytest.raises(ValueError, match="T must"):
        information_matrix(Fo, [[0, 1], [1, 0]], T[:, :2])
    with pytest.raises(ValueError, match="pairs"):
        information_matrix(Fo, [[0, 1]], T)
