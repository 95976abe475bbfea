"""CPU-side checks of the multiview synchronisation: the entry point's argument validation (returns before any HIP
call), the trajectory I/O of scripts/multiview_sync.py with the solve stubbed by the numpy oracle, pairwise_from_poses,
the oracle itself against ground truth, and the input conditions the GPU tests (test_gpu_sync.py) rely on."""
import os

import numpy as np
import pytest

from conftest import PKG
import sync_oracle as O

LIB = os.path.join(PKG, "libmvreg_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmvreg_hip.so not built")


# ------------------------------------------------------------------------------------------ the entry point's checks
def _call(L, S=1, max_frags=4, max_edges=3, anchor=0, irls=0, c=0.1, R=8, ws=None, ws_bytes=None, ptrs=8):
    """mvr_sync_poses with fake non-NULL device pointers (never dereferenced: every call here returns first)"""
    p = ptrs if ptrs else None
    need = L.mvr_sync_workspace_bytes(S, max_frags, max_edges)
    return L.mvr_sync_poses(p, p, p, None, max_edges, p, p, S, max_frags, max_edges, anchor, irls, c, c,
                            R if R else None, p, max_frags, None, None, None, None, p,
                            ws if ws is not None else p, need if ws_bytes is None else ws_bytes, None)


@needs_lib
def test_empty_and_invalid_calls():
    from lib import _native
    L = _native.lib()
    assert L.mvr_sync_workspace_bytes(1, 30, 435) >= (9 * 30 * 30 + 2 * 435) * 8
    # S = 0: MVR_OK before any pointer is read
    assert L.mvr_sync_poses(None, None, None, None, 0, None, None, 0, 30, 435, 0, 0, 0.1, 0.1, None, None, 0, None,
                            None, None, None, None, None, 0, None) == 0
    assert _call(L, max_frags=129) == -1                       # above MVR_SYNC_MAX_FRAGS
    assert _call(L, S=0, max_frags=129) == -1                  # scalars are validated before the empty short-cut
    assert _call(L, irls=-1) == -1
    assert _call(L, S=-1) == -1
    assert _call(L, max_edges=-1) == -1
    assert _call(L, anchor=4) == -1 and _call(L, anchor=-1) == -1
    assert _call(L, irls=1, c=0.0) == -1
    assert _call(L, ws_bytes=L.mvr_sync_workspace_bytes(1, 4, 3) - 1) == -1   # a workspace that is too small
    assert _call(L, R=0) == -1                                 # NULL R with S = 1
    assert _call(L, ptrs=0, R=8) == -1                         # NULL counts / status / edges


# ------------------------------------------------------------------------------------------------- Python surface
def _numpy_pairwise(R, t, pairs):
    out = []
    for i, j in pairs:
        Mi, Mj = np.eye(4), np.eye(4)
        Mi[:3, :3], Mi[:3, 3] = R[i], t[i]
        Mj[:3, :3], Mj[:3, 3] = R[j], t[j]
        out.append(np.linalg.inv(Mj) @ Mi)
    return np.asarray(out)


def test_pairwise_from_poses_matches_numpy_loop():
    import torch
    from lib.multiview import pairwise_from_poses
    sc = O.make_scene(7, O.complete_edges(7) + [(5, 2), (6, 0)], seed=21)
    want = _numpy_pairwise(sc["R_gt"], sc["t_gt"], sc["ij"])
    got = pairwise_from_poses(sc["R_gt"], sc["t_gt"], sc["ij"])
    assert isinstance(got, np.ndarray) and got.shape == (len(sc["ij"]), 4, 4)
    assert np.abs(got - want).max() < 1e-14
    # noise-free edges are exactly these transforms: x_j = R_k x_i + t_k
    assert np.abs(got[:, :3, :3] - sc["R_pair"]).max() < 1e-14 and np.abs(got[:, :3, 3] - sc["t_pair"]).max() < 1e-14
    got_t = pairwise_from_poses(torch.from_numpy(sc["R_gt"]), torch.from_numpy(sc["t_gt"]),
                                torch.from_numpy(sc["ij"]))
    assert torch.is_tensor(got_t) and np.abs(got_t.numpy() - want).max() < 1e-14


def test_weights_from_scores():
    import torch
    from lib.multiview import weights_from_scores
    s = torch.tensor([[0.9, 0.6, 0.1, 0.5], [0.0, 0.2, 0.3, 0.4]])
    assert weights_from_scores(s).tolist() == [0.5, 0.0]
    assert weights_from_scores(s, threshold=0.25).tolist() == [0.75, 0.5]


def test_sync_trajectory_io_roundtrip(tmp_path, monkeypatch):
    """traj.txt (T_log = inv(T), as the pairwise benchmark writes it) -> poses.txt + traj_sync.txt, the solve stubbed
    by the oracle: the inversion convention on the way in and on the way out, and the files' layout."""
    from lib.utils import read_trajectory, write_trajectory
    from scripts import multiview_sync as MS
    sc = O.make_scene(6, O.complete_edges(6), seed=22)
    E = len(sc["ij"])
    T = np.tile(np.eye(4), (E, 1, 1))
    T[:, :3, :3], T[:, :3, 3] = sc["R_pair"], sc["t_pair"]
    meta = [[str(i), str(j), True] for i, j in sc["ij"]]
    meta[3][2] = False                      # a pair the overlap gate rejected: the benchmark does not write it
    traj_file = str(tmp_path / "traj.txt")
    write_trajectory(np.linalg.inv(T), meta, traj_file)
    seen = {}

    def stub(R_pair, t_pair, pairs, n_frags, **kw):
        seen.update(R=np.asarray(R_pair), t=np.asarray(t_pair), pairs=np.asarray(pairs), kw=kw)
        return O.sync_oracle(R_pair, t_pair, pairs, n_frags, None, kw["anchor"], kw["irls_iters"], kw["c_rot"],
                             kw["c_trans"])
    monkeypatch.setattr(MS, "synchronize", stub)
    out_dir = str(tmp_path / "out")
    MS.main(["--traj", traj_file, "--n_fragments", "6", "--irls", "2", "--out", out_dir])
    keep = [k for k in range(E) if k != 3]
    # the solve saw the estimates themselves (log convention undone), in pair order, source -> target
    assert np.array_equal(seen["pairs"], sc["ij"][keep]) and seen["kw"]["irls_iters"] == 2
    assert np.abs(seen["R"] - sc["R_pair"][keep]).max() < 1e-10 and np.abs(seen["t"] - sc["t_pair"][keep]).max() < 1e-10
    keys, poses = read_trajectory(os.path.join(out_dir, "poses.txt"))
    assert [list(k) for k in keys] == [[str(i), str(i), "6"] for i in range(6)]
    assert np.abs(poses[:, :3, :3] - sc["R_gt"]).max() < 1e-9 and np.abs(poses[:, :3, 3] - sc["t_gt"]).max() < 1e-9
    assert np.array_equal(poses[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (6, 1)))
    keys2, traj2 = read_trajectory(os.path.join(out_dir, "traj_sync.txt"))
    keys1, traj1 = read_trajectory(traj_file)
    assert np.array_equal(keys1, keys2) and len(keys2) == E - 1
    # noise-free input: the synchronised pairwise estimates are the input estimates, still in the log convention
    assert np.abs(traj2 - traj1).max() < 1e-9
    assert np.abs(traj2 - np.linalg.inv(T)[keep]).max() < 1e-9


# --------------------------------------------------------------------------------------- the oracle vs ground truth
@pytest.mark.parametrize("name", O.NOISE_FREE + ("two_components",))
def test_oracle_recovers_noise_free_poses(name):
    sc, irls, out = O.case(name)
    member = out["member"].astype(bool)
    er, et = O.pose_error(out, sc, member)
    print("%s: rot %.3g trans %.3g" % (name, er, et))
    assert er < 1e-9 and et < 1e-9
    assert out["res_rot"].max() < 1e-9 or name == "two_components"
    if name == "two_components":
        assert out["status"] == 1 and member.tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
        assert np.array_equal(out["R"][3:], np.tile(np.eye(3), (5, 1, 1))) and not out["t"][3:].any()
        assert not out["weights"][3:].any() and np.array_equal(out["weights"][:3], np.ones(3))
    else:
        assert out["status"] == 0 and member.all()


@pytest.mark.parametrize("name", ["complete30", "ring12", "chain12_reversed"])
def test_oracle_noise_free_random_weights_change_nothing(name):
    sc, irls, out = O.case(name)
    w = np.random.default_rng(5).uniform(0.2, 1.0, len(sc["ij"]))
    out_w = O.sync_oracle(sc["R_pair"], sc["t_pair"], sc["ij"], sc["n"], w, sc["anchor"])
    assert np.abs(out_w["R"] - out["R"]).max() < 1e-9 and np.abs(out_w["t"] - out["t"]).max() < 1e-9
    assert O.pose_error(out_w, sc)[0] < 1e-9 and O.pose_error(out_w, sc)[1] < 1e-9


def test_oracle_edge_cases():
    one = O.sync_oracle(np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0, 2)), 1)
    assert one["status"] == 0 and one["member"].tolist() == [1] and np.array_equal(one["R"][0], np.eye(3))
    sc = O.case("n3")[0]
    far = O.sync_oracle(sc["R_pair"], sc["t_pair"], sc["ij"], 3, anchor=3)
    assert far["status"] == 5 and not far["member"].any() and np.array_equal(far["R"], np.tile(np.eye(3), (3, 1, 1)))
    # ignored edges: the result of the run without them, status bit 4, weight and residuals 0
    bad, _, out = O.case("bad_edges")
    clean = O.sync_oracle(bad["R_pair"][:-2], bad["t_pair"][:-2], bad["ij"][:-2], bad["n"], bad["w"][:-2])
    assert out["status"] == 4 and clean["status"] == 0
    assert np.array_equal(out["R"], clean["R"]) and np.array_equal(out["t"], clean["t"])
    assert not out["weights"][-2:].any() and not out["res_rot"][-2:].any()
    # the ignored edge was the only way to fragment 2: the edge test decides the component
    cut = O.case("cut_by_bad_edge")[2]
    assert cut["status"] == 5 and cut["member"].tolist() == [1, 1, 0] and cut["weights"].tolist() == [1.0, 0.0, 0.0]
    # one fragment, two edges that cannot count: on the seam between the edge test and the single-fragment return
    sc = O.N1_BAD_EDGES
    n1 = O.sync_oracle(sc["R_pair"], sc["t_pair"], sc["ij"], 1, sc["w"])
    assert n1["status"] == 4 and n1["member"].tolist() == [1] and not n1["weights"].any()
    assert np.array_equal(n1["R"][0], np.eye(3)) and not n1["t"].any()


def test_wrapper_argument_rules_without_a_device():
    """every shape and count rule of synchronize is a ValueError, raised before a device is asked for"""
    from lib.multiview import synchronize
    sc = O.make_scene(4, O.complete_edges(4)[:5], seed=23)
    R, t, ij = sc["R_pair"], sc["t_pair"], sc["ij"]
    assert len(ij) == 5
    for args, kw in ((([R], [t, t], [ij], [4]), {}),                          # per-scene lists of unequal length
                     (([R], [t], [ij], [4]), dict(weights=[sc["w"], sc["w"]])),
                     (([R], [t[:1]], [ij], [4]), {}),                         # one t_pair row for five edges
                     (([R], [t], [ij], [4]), dict(weights=[np.ones(1)])),     # one weight for five edges
                     (([R], [t], [ij[:-1]], [4]), {}),                        # pairs with a row short
                     ((R, t, ij[:-1], 4), {}),
                     ((R[None], t[None], ij[None, :-1], [4]), {}),
                     ((R, t[:1], ij, 4), {}),
                     ((R, t, ij, 4), dict(weights=np.ones(1))),
                     ((R.reshape(-1, 9), t, ij, 4), {}),                      # R_pair [E,9]
                     ((R[None], t[None], ij[None], [4, 4]), {}),              # n_frags of the wrong length
                     (([R], [t], [ij], [4, 4]), {}),
                     ((R[None], t[None], ij[None], [4]), dict(n_edges=[6])),  # n_edges above E
                     ((R[None], t[None], ij[None], [4]), dict(n_edges=[5, 5])),
                     ((R, t, ij, 129), {}),                                   # n_frags above MAX_FRAGS
                     ((R, t, ij, -1), {}),
                     ((R, t, ij, 4), dict(anchor=4)),                         # anchor outside
                     ((R, t, ij, 4), dict(anchor=-1))):
        with pytest.raises(ValueError, match="synchronize: "):
            synchronize(*args, **kw)


# ------------------------------------------------------------------- the input conditions the GPU tests rely on
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_spectral_gap_of_every_compared_case(name):
    """1e-9 against the oracle is a fair bound only where the bottom three eigenvalues are separated from the
    fourth: lambda_4 - lambda_3 >= 1e-3 lambda_max in every pass of every case a GPU test compares."""
    sc, irls, out = O.case(name)
    gaps = [O.spectral_gap(s) for s in out["spectra"]]
    print(name, ["%.3g" % g for g in gaps])
    assert len(gaps) == irls + 1 and min(gaps) >= 1e-3


def test_spectral_gap_fp32_inputs():
    """the Python-surface GPU test runs the outlier scene from fp32 inputs: the same condition there"""
    sc, irls, _ = O.case("outliers30")
    out = O.sync_oracle(sc["R_pair"].astype(np.float32), sc["t_pair"].astype(np.float32), sc["ij"], sc["n"], None,
                        0, irls, return_spectrum=True)
    assert min(O.spectral_gap(s) for s in out["spectra"]) >= 1e-3
    assert max(O.pose_error(out, sc)) < O.OUTLIER_BOUND


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_outlier_scene_needs_irls(seed):
    """30 fragments, 30 % of the 435 pairs replaced by random transforms, sigma 0.01, c 0.1: five passes land within
    0.05 of ground truth (rotation Frobenius and translation), the plain closed form does not"""
    sc = O.make_scene(30, O.complete_edges(30), seed, 0.01, 0.01, 0.3)
    assert sc["outlier"].sum() == round(0.3 * 435)
    plain = O.sync_oracle(sc["R_pair"], sc["t_pair"], sc["ij"], 30, sc["w"])
    irls = O.sync_oracle(sc["R_pair"], sc["t_pair"], sc["ij"], 30, sc["w"], irls_iters=5)
    print("seed %d: plain %s irls %s" % (seed, O.pose_error(plain, sc), O.pose_error(irls, sc)))
    assert max(O.pose_error(irls, sc)) < O.OUTLIER_BOUND
    assert not max(O.pose_error(plain, sc)) < O.OUTLIER_BOUND
    # the outlier edges end below every clean edge
    assert irls["weights"][sc["outlier"]].max() < irls["weights"][~sc["outlier"]].min()


def test_outlier_scene_of_the_gpu_test():
    sc, irls, out = O.case("outliers30")
    assert irls == 5 and max(O.pose_error(out, sc)) < O.OUTLIER_BOUND
    assert out["weights"][sc["outlier"]].max() < out["weights"][~sc["outlier"]].min()
    # the synchronised estimate of an outlier edge is within the bound of that edge's ground truth
    k = int(np.nonzero(sc["outlier"])[0][0])
    got = _numpy_pairwise(out["R"], out["t"], sc["ij"][k:k + 1])[0]
    want = _numpy_pairwise(sc["R_gt"], sc["t_gt"], sc["ij"][k:k + 1])[0]
    assert np.linalg.norm(got[:3, :3] - want[:3, :3]) < O.OUTLIER_BOUND
    assert np.linalg.norm(got[:3, 3] - want[:3, 3]) < O.OUTLIER_BOUND
    assert np.linalg.norm(sc["R_pair"][k] - want[:3, :3]) > 0.5       # the input estimate was an outlier
