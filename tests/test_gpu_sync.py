"""GPU tests of the multiview pose synchronisation (csrc/sync.hip mvr_sync_poses, lib.multiview) against the numpy
oracle (tests/sync_oracle.py) and ground truth.  The reference holds nothing for this stage: parity is pinned to the
closed form the oracle restates.  Tolerance against the oracle: 1e-9 on R, t, residuals and final weights (the
project's fp64 bound); member and status equal.  test_sync_host.py checks the conditions these comparisons rely on
(spectral gap of every case, the outlier scene's behaviour in the oracle alone)."""
import numpy as np
import pytest

import sync_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = ("R", "t", "weights", "res_rot", "res_trans")


def run_gpu(gpu, scenes, anchor=0, irls=0, c_rot=0.1, c_trans=0.1, max_frags=None, max_edges=None, weights=True):
    """mvr_sync_poses on a padded batch of scenes (dicts of make_scene) -> one result dict of numpy arrays per scene"""
    import torch
    from lib import _native as N
    S = len(scenes)
    F = max_frags or max(s["n"] for s in scenes)
    Em = max_edges or max(len(s["ij"]) for s in scenes)
    Rp = np.zeros((S, Em, 9))
    tp = np.zeros((S, Em, 3))
    ij = np.zeros((S, Em, 2), np.int32)
    w = np.zeros((S, Em))
    for k, s in enumerate(scenes):
        e = len(s["ij"])
        Rp[k, :e], tp[k, :e], ij[k, :e], w[k, :e] = s["R_pair"].reshape(-1, 9), s["t_pair"], s["ij"], s["w"]
    dev = [torch.from_numpy(x).to(gpu) for x in (Rp, tp, ij, w)]
    n_e = torch.tensor([len(s["ij"]) for s in scenes], dtype=torch.int32, device=gpu)
    n_f = torch.tensor([s["n"] for s in scenes], dtype=torch.int32, device=gpu)
    R = torch.full((S, F, 9), 7.0, dtype=torch.float64, device=gpu)
    t = torch.full((S, F, 3), 7.0, dtype=torch.float64, device=gpu)
    member = torch.full((S, F), 7, dtype=torch.int32, device=gpu)
    wo, er, et = (torch.full((S, Em), 7.0, dtype=torch.float64, device=gpu) for _ in range(3))
    status = torch.full((S,), 7, dtype=torch.int32, device=gpu)
    L = N.lib()
    ws = torch.empty(L.mvr_sync_workspace_bytes(S, F, Em), dtype=torch.uint8, device=gpu)
    rc = L.mvr_sync_poses(N.ptr(dev[0]), N.ptr(dev[1]), N.ptr(dev[2]), N.ptr(dev[3]) if weights else None, Em,
                          N.ptr(n_e), N.ptr(n_f), S, F, Em, anchor, irls, c_rot, c_trans, N.ptr(R), N.ptr(t), F,
                          N.ptr(member), N.ptr(wo), N.ptr(er), N.ptr(et), N.ptr(status), N.ptr(ws), ws.numel(),
                          N.stream())
    assert rc == 0
    torch.cuda.synchronize()
    out = []
    for k, s in enumerate(scenes):
        n, e = s["n"], len(s["ij"])
        out.append({"R": R[k, :n].cpu().numpy().reshape(n, 3, 3), "t": t[k, :n].cpu().numpy(),
                    "member": member[k, :n].cpu().numpy(), "weights": wo[k, :e].cpu().numpy(),
                    "res_rot": er[k, :e].cpu().numpy(), "res_trans": et[k, :e].cpu().numpy(),
                    "status": int(status[k].item())})
    return out


def assert_matches_oracle(got, want, what):
    diffs = {k: float(np.abs(got[k] - want[k]).max()) if got[k].size else 0.0 for k in KEYS}
    print(what, "status", got["status"], "max |gpu - oracle|:", " ".join("%s %.3g" % kv for kv in diffs.items()))
    assert got["status"] == want["status"], what
    assert np.array_equal(got["member"], want["member"]), what
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.isfinite(got[k]).all(), (what, k)
        assert diffs[k] <= TOL, (what, k, diffs[k])


def gpu_case(gpu, name, **kw):
    sc, irls, want = O.case(name)
    got = run_gpu(gpu, [sc], anchor=sc["anchor"], irls=irls, **kw)[0]
    return sc, got, want


@pytest.mark.parametrize("name", O.NOISE_FREE)
def test_noise_free_recovery(gpu, name):
    sc, got, want = gpu_case(gpu, name)
    assert_matches_oracle(got, want, name)
    er, et = O.pose_error(got, sc)
    print(name, "vs ground truth: rot %.3g trans %.3g" % (er, et))
    assert er <= TOL and et <= TOL and got["status"] == 0 and got["member"].all()


@pytest.mark.parametrize("name", ["complete30_noisy", "ring12_noisy", "cut_by_bad_edge"])
def test_noisy_scene_matches_oracle(gpu, name):
    sc, got, want = gpu_case(gpu, name)
    assert_matches_oracle(got, want, name)


def test_unit_weights_when_w_is_null(gpu):
    sc, irls, _ = O.case("ring12_noisy")
    want = O.sync_oracle(sc["R_pair"], sc["t_pair"], sc["ij"], sc["n"], None)
    got = run_gpu(gpu, [sc], weights=False)[0]
    assert_matches_oracle(got, want, "ring12_noisy, w NULL")


def test_non_zero_anchor(gpu):
    sc, got, want = gpu_case(gpu, "anchor7")
    assert sc["anchor"] == 7
    assert np.array_equal(got["R"][7], np.eye(3)) and np.array_equal(got["t"][7], np.zeros(3))
    assert_matches_oracle(got, want, "anchor7")


def test_irls_rejects_outliers(gpu):
    sc, got, want = gpu_case(gpu, "outliers30")
    assert_matches_oracle(got, want, "outliers30 irls 5")
    er, et = O.pose_error(got, sc)
    print("outliers30 vs ground truth: rot %.3g trans %.3g" % (er, et))
    assert er < O.OUTLIER_BOUND and et < O.OUTLIER_BOUND
    assert got["weights"][sc["outlier"]].max() < got["weights"][~sc["outlier"]].min()


def test_components(gpu):
    sc, got, want = gpu_case(gpu, "two_components")
    assert got["status"] & 1 and got["member"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert np.array_equal(got["R"][3:], np.tile(np.eye(3), (5, 1, 1))) and not got["t"][3:].any()
    assert_matches_oracle(got, want, "two_components")
    er, et = O.pose_error(got, sc, got["member"])
    assert er <= TOL and et <= TOL


def test_bad_edges_are_ignored(gpu):
    sc, got, want = gpu_case(gpu, "bad_edges")
    assert got["status"] & 4
    assert_matches_oracle(got, want, "bad_edges")
    clean = O.sync_oracle(sc["R_pair"][:-2], sc["t_pair"][:-2], sc["ij"][:-2], sc["n"], sc["w"][:-2])
    assert np.abs(got["R"] - clean["R"]).max() <= TOL and np.abs(got["t"] - clean["t"]).max() <= TOL
    assert not got["weights"][-2:].any() and not got["res_rot"][-2:].any() and not got["res_trans"][-2:].any()


def test_anchor_outside_the_scene(gpu):
    sc = O.case("n3")[0]
    big = O.case("ring12")[0]
    got = run_gpu(gpu, [sc, big], anchor=5)          # anchor 5: fine for the ring of 12, outside the scene of 3
    want = O.sync_oracle(sc["R_pair"], sc["t_pair"], sc["ij"], 3, sc["w"], anchor=5)
    assert_matches_oracle(got[0], want, "n3, anchor 5")
    assert got[0]["status"] & 4 and np.array_equal(got[0]["R"], np.tile(np.eye(3), (3, 1, 1)))
    want = O.sync_oracle(big["R_pair"], big["t_pair"], big["ij"], 12, big["w"], anchor=5)
    assert_matches_oracle(got[1], want, "ring12, anchor 5")


def test_batch_is_bit_equal_to_single_scenes(gpu):
    one = {"n": 1, "anchor": 0, "R_pair": np.zeros((0, 3, 3)), "t_pair": np.zeros((0, 3)),
           "ij": np.zeros((0, 2), np.int64), "w": np.zeros(0)}
    scenes = [O.case("ring12_noisy")[0], one, O.case("outliers30")[0], O.N1_BAD_EDGES]
    batch = run_gpu(gpu, scenes, irls=2)
    assert batch[1]["status"] == 0 and batch[1]["member"].tolist() == [1]
    assert np.array_equal(batch[1]["R"][0], np.eye(3)) and not batch[1]["t"].any()
    for k, sc in enumerate(scenes):
        alone = run_gpu(gpu, [sc], irls=2)[0]
        assert alone["status"] == batch[k]["status"] and np.array_equal(alone["member"], batch[k]["member"])
        for key in KEYS:
            assert np.array_equal(alone[key], batch[k][key]), (k, key)
    want = O.sync_oracle(scenes[0]["R_pair"], scenes[0]["t_pair"], scenes[0]["ij"], 12, scenes[0]["w"], irls_iters=2)
    assert_matches_oracle(batch[0], want, "ring12_noisy in a batch, irls 2")
    # one fragment with edges that cannot count: between the edge test and the single-fragment return
    bad = scenes[3]
    want = O.sync_oracle(bad["R_pair"], bad["t_pair"], bad["ij"], 1, bad["w"], irls_iters=2)
    assert want["status"] == 4 and batch[3]["status"] == 4 and batch[3]["member"].tolist() == [1]
    assert_matches_oracle(batch[3], want, "n1_bad_edges in a batch, irls 2")
    assert not batch[3]["weights"].any() and np.array_equal(batch[3]["R"][0], np.eye(3)) and not batch[3]["t"].any()


@pytest.mark.parametrize("name", ["complete64", "complete42", "complete43"])
def test_sizes(gpu, name):
    """64 fragments / 2016 edges (matrix in the workspace), and either side of the switch from the LDS-resident
    matrix (max_frags <= 42) to the workspace-resident one"""
    sc, got, want = gpu_case(gpu, name)
    assert_matches_oracle(got, want, name)


def test_lds_and_workspace_paths_agree(gpu):
    """the same scene through both instantiations (max_frags 30 -> LDS, padded to 64 -> workspace)"""
    sc, irls, want = O.case("complete30_noisy")
    a = run_gpu(gpu, [sc])[0]
    b = run_gpu(gpu, [sc], max_frags=64, max_edges=500)[0]
    assert_matches_oracle(b, want, "complete30_noisy, max_frags 64")
    for key in KEYS:
        assert np.abs(a[key] - b[key]).max() <= TOL


def test_python_surface_fp32_inputs(gpu):
    import torch
    from lib.multiview import synchronize, pairwise_from_poses
    from lib.utils import pair_index
    sc, irls, _ = O.case("outliers30")
    pairs = pair_index(30, gpu)
    assert np.array_equal(pairs.cpu().numpy(), sc["ij"])
    R32 = torch.from_numpy(sc["R_pair"]).float().to(gpu)
    t32 = torch.from_numpy(sc["t_pair"]).float().to(gpu)
    out = synchronize(R32, t32, pairs, 30, irls_iters=irls)
    assert all(torch.is_tensor(v) and v.device.type == "cuda" for v in out.values())
    assert out["R"].shape == (30, 3, 3) and out["R"].dtype == torch.float64 and out["status"].dim() == 0
    # the oracle on the fp64 conversion of the same fp32 inputs: only the conversion differs from the fp64 cases
    want = O.sync_oracle(R32.cpu().numpy().astype(np.float64), t32.cpu().numpy().astype(np.float64), sc["ij"], 30,
                         None, 0, irls)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["status"] = int(got["status"])
    assert_matches_oracle(got, want, "synchronize(fp32 torch)")
    k = int(np.nonzero(sc["outlier"])[0][0])
    T = pairwise_from_poses(out["R"], out["t"], pairs[k:k + 1])[0].cpu().numpy()
    i, j = sc["ij"][k]
    R_gt = sc["R_gt"][j].T @ sc["R_gt"][i]
    t_gt = sc["R_gt"][j].T @ (sc["t_gt"][i] - sc["t_gt"][j])
    assert np.linalg.norm(T[:3, :3] - R_gt) < O.OUTLIER_BOUND and np.linalg.norm(T[:3, 3] - t_gt) < O.OUTLIER_BOUND
    # numpy lists of scenes: a batch, back on the host
    small = O.case("ring12_noisy")[0]
    both = synchronize([sc["R_pair"], small["R_pair"]], [sc["t_pair"], small["t_pair"]], [sc["ij"], small["ij"]],
                       [30, 12], weights=[sc["w"], small["w"]])
    assert isinstance(both["R"], np.ndarray) and both["R"].shape == (2, 30, 3, 3) and both["status"].tolist() == [0, 0]
    want = O.case("ring12_noisy")[2]
    assert np.abs(both["R"][1, :12] - want["R"]).max() <= TOL and np.abs(both["t"][1, :12] - want["t"]).max() <= TOL
    assert np.array_equal(both["R"][1, 12:], np.tile(np.eye(3), (18, 1, 1)))
    # the three input forms: per-scene lists, a padded batch with n_edges, and each scene alone, byte for byte
    scs = [O.case(n)[0] for n in ("n2", "n3", "cut_by_bad_edge")]
    nf, ne = [s["n"] for s in scs], [len(s["ij"]) for s in scs]
    keys = ("R_pair", "t_pair", "ij")
    lists = synchronize(*([s[k] for s in scs] for k in keys), nf, weights=[s["w"] for s in scs], irls_iters=2)

    def padded(k):
        out = np.full((3, max(ne)) + scs[0][k].shape[1:], 7, scs[0][k].dtype)    # the padding is never read
        for i, s in enumerate(scs):
            out[i, :ne[i]] = s[k]
        return out
    pad = synchronize(*(padded(k) for k in keys), nf, weights=padded("w"), irls_iters=2, n_edges=ne)
    assert lists["status"].tolist() == [0, 0, 5] and lists["member"].tolist() == [[1, 1, 0], [1, 1, 1], [1, 1, 0]]
    for i, s in enumerate(scs):
        alone = synchronize(*(s[k] for k in keys), nf[i], weights=s["w"], irls_iters=2)
        for k in ("R", "t", "member", "weights", "status"):
            n = {"R": nf[i], "t": nf[i], "member": nf[i], "weights": ne[i]}.get(k)
            a, b = (np.ascontiguousarray(x[k][i] if n is None else x[k][i, :n]) for x in (lists, pad))
            assert a.tobytes() == b.tobytes() == alone[k].tobytes(), (i, k)
