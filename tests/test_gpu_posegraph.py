"""GPU pose-graph refinement (csrc/posegraph.hip mvr_posegraph_optimize, lib.multiview.optimize_pose_graph) against
the numpy oracle (tests/posegraph_oracle.py) on its seeded scenes (posegraph_oracle.cases()).

iters, status, member and the accept / reject pattern of the trace: exactly (test_posegraph_host.py asserts that no
decision of any case is within 1e-6 of its threshold).  Poses and costs: the oracle runs twice per scene, with
np.linalg.cholesky and with np.linalg.solve; the two differ only in the rounding of the solve, and the kernel's
blocked Cholesky is a third variant, so the bound is 100 x the largest difference between the two runs (poses:
absolute over the entries of R and t; costs and trace: relative to the initial cost), and 1e-12 where they agree bit
for bit.  For the costs the two runs' difference is one of two measured floors: they evaluate a given set of poses
with the same code, so it says nothing about the evaluation's own rounding, which the kernel does in another order.
The second floor measures that: the oracle's cost of the initial and of the final poses, re-evaluated with the edges
shuffled and the products associated the other way round (posegraph_oracle.cost_evaluation_floor).  The cost bound is
100 x the larger floor, 1e-12 where both are zero.  The measured floors are in DESIGN.md 4.22.  The kernel keeps the
matrix in the workspace at every size: there is no LDS / workspace boundary to straddle; 256 | 257 edges is the
boundary of its endpoint staging."""
import functools

import numpy as np
import pytest

import posegraph_oracle as PO

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle(name):
    sc, kw = PO.cases()[name]
    a, b = PO.run(sc, **kw), PO.run(sc, solver="solve", **kw)
    assert a["accepted"] == b["accepted"] and a["iters"] == b["iters"] and a["status"] == b["status"], name
    c0 = max(a["cost"][0], 1e-300)
    floor_pose = max(np.abs(a["R"] - b["R"]).max(initial=0.0), np.abs(a["t"] - b["t"]).max(initial=0.0))
    floor_cost = np.abs(a["trace"] - b["trace"]).max() / c0
    anchor = kw.get("anchor", 0)
    floor_eval = max(PO.cost_evaluation_floor(sc, sc["R0"], sc["t0"], anchor),
                     PO.cost_evaluation_floor(sc, a["R"], a["t"], anchor)) / c0
    floor_cost = max(floor_cost, floor_eval)
    return a, 100.0 * floor_pose if floor_pose > 0 else 1e-12, 100.0 * floor_cost if floor_cost > 0 else 1e-12


def _gpu(sc, **kw):
    from lib.multiview import optimize_pose_graph
    return optimize_pose_graph(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"],
                               return_trace=True, **kw)


def _pattern(trace, iters):
    """per trial: True where the held cost fell"""
    return [bool(trace[k + 1] < trace[k]) for k in range(iters)]


NAMES = sorted(PO.cases())


@pytest.mark.parametrize("name", NAMES)
def test_matches_oracle(gpu, name):
    sc, kw = PO.cases()[name]
    want, tol_pose, tol_cost = _oracle(name)
    got = _gpu(sc, **kw)
    n, k, c0 = len(sc["R0"]), want["iters"], max(want["cost"][0], 1e-300)
    d_pose = max(np.abs(got["R"] - want["R"]).max(initial=0.0), np.abs(got["t"] - want["t"]).max(initial=0.0))
    d_cost = max(np.abs(got["trace"] - want["trace"]).max(), np.abs(got["cost"] - want["cost"]).max()) / c0
    print("%s: N %d, E %d, trials %d, status %d, cost %.6g -> %.6g; |d pose| %.3g (bound %.3g), |d cost| / c0 %.3g "
          "(bound %.3g)" % (name, n, len(sc["ij"]), k, want["status"], want["cost"][0], want["cost"][1], d_pose,
                            tol_pose, d_cost, tol_cost))
    assert int(got["iters"]) == k and int(got["status"]) == want["status"]
    np.testing.assert_array_equal(got["member"], want["member"])
    assert got["trace"].shape == (kw.get("max_iters", 20) + 1,)
    assert (got["trace"][k + 1:] == -1.0).all() and (got["trace"][:k + 1] >= 0).all()
    assert _pattern(got["trace"], k) == want["accepted"] == _pattern(want["trace"], k)
    assert got["cost"][0] == got["trace"][0] and got["cost"][1] == got["trace"][k]
    assert d_pose <= tol_pose and d_cost <= tol_cost
    held = [f for f in range(n) if not want["member"][f] or f == kw.get("anchor", 0)]
    assert got["R"][held].tobytes() == sc["R0"][held].tobytes() and got["t"][held].tobytes() == sc["t0"][held].tobytes()


def test_invalid_scenes_copy_their_poses(gpu):
    from lib.multiview import optimize_pose_graph
    sc = PO.cases()["n3_noisy"][0]
    bad = dict(sc, t0=sc["t0"].copy())
    bad["t0"][2, 1] = np.nan
    big = PO.cases()["anchor3"][0]

    def lists(scs, key):
        return [s[key] for s in scs]
    scs = [big, sc, bad, big]
    out = optimize_pose_graph(*(lists(scs, k) for k in ("R0", "t0", "R_pair", "t_pair", "ij", "info", "w")), anchor=3,
                              max_iters=2, tol_cost=0.0, tol_step=0.0, return_trace=True)
    assert out["status"].tolist() == [0, 5, 5, 0]                   # anchor 3 >= 3 fragments; a NaN in a pose
    for s in (1, 2):
        assert not out["member"][s].any() and out["iters"][s] == 0 and not out["cost"][s].any()
        assert (out["trace"][s] == -1.0).all()
        assert out["R"][s, :3].tobytes() == scs[s]["R0"].tobytes()
        assert out["t"][s, :3].tobytes() == scs[s]["t0"].tobytes()
    alone = _gpu(big, anchor=3, max_iters=2, tol_cost=0.0, tol_step=0.0)
    for s in (0, 3):
        for key in alone:
            assert np.ascontiguousarray(out[key][s]).tobytes() == alone[key].tobytes(), (s, key)


def test_a_scene_alone_and_in_a_ragged_batch(gpu):
    from lib.multiview import optimize_pose_graph
    C = PO.cases()
    kw = dict(max_iters=3, tol_cost=0.0, tol_step=0.0)
    main = C["n30_noisy"][0]
    alone = _gpu(main, **kw)
    assert int(alone["iters"]) == 3 and int(alone["status"]) == 0
    others = [C[n][0] for n in ("n3_noisy", "edges_129", "n1", "disconnected", "reject", "n43_noisy", "bad_edges")]
    for pos in (0, 3, 7):
        scs = others[:pos] + [main] + others[pos:]
        assert len(scs) == 8
        out = optimize_pose_graph(*([s[k] for s in scs] for k in ("R0", "t0", "R_pair", "t_pair", "ij", "info", "w")),
                                  return_trace=True, **kw)
        assert out["R"].shape == (8, 43, 3, 3) and out["trace"].shape == (8, 4)
        for key in ("R", "t", "member"):
            assert np.ascontiguousarray(out[key][pos, :30]).tobytes() == alone[key].tobytes(), (pos, key)
        for key in ("cost", "iters", "status", "trace"):
            assert np.ascontiguousarray(out[key][pos]).tobytes() == alone[key].tobytes(), (pos, key)
        # the rows past a scene's fragments keep what they held: zero padding
        k1 = [i for i, s in enumerate(scs) if s is C["n1"][0]][0]
        assert not out["R"][k1, 1:].any() and out["member"][k1].tolist() == [1] + [0] * 42


def test_python_surface(gpu):
    import torch
    from lib.multiview import optimize_pose_graph
    sc, kw = PO.cases()["anchor3"]
    ref = _gpu(sc, **kw)
    a = (sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"])
    dev = optimize_pose_graph(*(torch.from_numpy(x).to(gpu) for x in a), return_trace=True, **kw)
    assert all(torch.is_tensor(v) and v.device.type == "cuda" for v in dev.values())
    assert dev["R"].shape == (8, 3, 3) and dev["cost"].shape == (2,) and dev["iters"].dtype == torch.int32
    for key in ref:
        assert dev[key].cpu().numpy().tobytes() == ref[key].tobytes(), key
    # padded batch with n_frags / n_edges, t_pair [E,3,1], info [E,36], host torch in -> host torch out, no trace
    pad = optimize_pose_graph(torch.from_numpy(np.concatenate([sc["R0"], np.zeros((2, 3, 3))]))[None],
                              torch.from_numpy(np.concatenate([sc["t0"], np.zeros((2, 3))]))[None],
                              torch.from_numpy(sc["R_pair"])[None], torch.from_numpy(sc["t_pair"])[None, :, :, None],
                              torch.from_numpy(sc["ij"])[None], torch.from_numpy(sc["info"]).reshape(1, -1, 36),
                              torch.from_numpy(sc["w"])[None], n_frags=[8], n_edges=[len(sc["ij"])], **kw)
    assert "trace" not in pad and all(torch.is_tensor(v) and v.device.type == "cpu" for v in pad.values())
    assert pad["R"].shape == (1, 10, 3, 3) and pad["R"][0, :8].numpy().tobytes() == ref["R"].tobytes()
    assert pad["cost"][0].numpy().tobytes() == ref["cost"].tobytes()
    # weights None = all ones; fp32 inputs are taken to fp64
    ones = _gpu(dict(sc, w=np.ones(len(sc["ij"]))), **kw)
    none = optimize_pose_graph(*a[:6], None, return_trace=True, **kw)
    for key in ones:
        assert none[key].tobytes() == ones[key].tobytes(), key
    f32 = optimize_pose_graph(*(x.astype(np.float32) if x.dtype == np.float64 else x for x in a), **kw)
    f64 = optimize_pose_graph(*(x.astype(np.float32).astype(np.float64) if x.dtype == np.float64 else x for x in a),
                              **kw)
    assert f32["R"].dtype == np.float64 and f32["R"].tobytes() == f64["R"].tobytes()
    # the three input forms: per-scene lists, a padded batch with n_frags / n_edges, and each scene alone
    scs = [PO.cases()[n][0] for n in ("n2_exact", "n3_noisy", "cut_by_bad_edge")]
    nf, ne = [len(s["R0"]) for s in scs], [len(s["ij"]) for s in scs]
    keys = ("R0", "t0", "R_pair", "t_pair", "ij", "info", "w")
    lists = optimize_pose_graph(*([s[k] for s in scs] for k in keys), **PO.TWO)

    def padded(k):
        count = nf if k in ("R0", "t0") else ne
        out = np.full((3, max(count)) + scs[0][k].shape[1:], 7, scs[0][k].dtype)   # the padding is never read
        for i, s in enumerate(scs):
            out[i, :count[i]] = s[k]
        return out
    pad = optimize_pose_graph(*(padded(k) for k in keys), n_frags=nf, n_edges=ne, **PO.TWO)
    assert lists["status"].tolist() == [0, 0, 5] and lists["member"][2].tolist() == [1, 1, 0]
    for i, s in enumerate(scs):
        alone = optimize_pose_graph(*(s[k] for k in keys), **PO.TWO)
        for k in alone:
            n = nf[i] if k in ("R", "t", "member") else None
            x, y = (np.ascontiguousarray(o[k][i] if n is None else o[k][i, :n]) for o in (lists, pad))
            assert x.tobytes() == y.tobytes() == alone[k].tobytes(), (i, k)
    empty = optimize_pose_graph([], [], [], [], [], [])
    assert empty["R"].shape == (0, 0, 3, 3) and empty["status"].shape == (0,)


def test_end_to_end_on_the_four_fragment_scene(gpu):
    """icp_refine from the perturbed starts -> information_matrix -> synchronize(irls_iters=5) -> optimize_pose_graph.
    The error against the scene's ground truth is printed beside the synchronised poses' error, not asserted: nothing
    guarantees that it improves on every scene."""
    import icp_oracle as O
    from lib.icp import icp_refine, information_matrix
    from lib.multiview import optimize_pose_graph, synchronize
    from lib.overlap import FragmentOverlap
    fo = FragmentOverlap(O.scene4()[0], "FCGF", 0.025)
    T0 = O.scene4_starts(O.TWELVE, O.scene4_centroids())
    icp = icp_refine(fo, O.TWELVE, T0, max_iters=30)
    info = information_matrix(fo, O.TWELVE, icp["T"])
    np.testing.assert_array_equal(info["n_corr"], icp["n_corr"])
    assert (info["status"] == 0).all() and (info["info"][:, 0, 0] == icp["n_corr"]).all()
    Rp, tp = icp["T"][:, :3, :3], icp["T"][:, :3, 3]
    sync = synchronize(Rp, tp, O.TWELVE, 4, irls_iters=5)
    assert sync["status"] == 0 and sync["member"].all()
    kw = dict(max_iters=2, tol_cost=0.0, tol_step=0.0)
    got = optimize_pose_graph(sync["R"], sync["t"], Rp, tp, O.TWELVE, info["info"], sync["weights"], return_trace=True,
                              **kw)
    want = PO.optimize(sync["R"], sync["t"], Rp, tp, np.asarray(O.TWELVE), info["info"], sync["weights"], **kw)
    other = PO.optimize(sync["R"], sync["t"], Rp, tp, np.asarray(O.TWELVE), info["info"], sync["weights"],
                        solver="solve", **kw)
    margins = np.asarray(want["margins"])
    floor = max(np.abs(want["R"] - other["R"]).max(), np.abs(want["t"] - other["t"]).max())
    bound = 100.0 * floor if floor > 0 else 1e-12
    d = max(np.abs(got["R"] - want["R"]).max(), np.abs(got["t"] - want["t"]).max())
    poses = O.scene4()[1]
    gt = [np.linalg.inv(poses[0]) @ p for p in poses]              # in the anchor's frame

    def err(R, t):
        return PO.pose_error(R, t, [g[:3, :3] for g in gt], [g[:3, 3] for g in gt])
    print("cost %.6g -> %.6g over %s (margins %s); |d pose| vs oracle %.3g (bound %.3g)"
          % (got["cost"][0], got["cost"][1], "".join("A" if x else "r" for x in want["accepted"]),
             " ".join("%.2g" % m for m in margins[:, 0]), d, bound))
    print("error against ground truth (rad, m): synchronised %.3g / %.3g, refined %.3g / %.3g"
          % (err(sync["R"], sync["t"]) + err(got["R"], got["t"])))
    assert got["cost"][1] <= got["cost"][0]
    assert int(got["status"]) == want["status"] and int(got["iters"]) == want["iters"]
    assert margins[:, 0].min() >= 1e-6                             # no trial of this run is decided by rounding
    assert _pattern(got["trace"], 2) == want["accepted"]
    assert d <= bound
