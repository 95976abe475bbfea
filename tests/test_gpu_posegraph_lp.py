"""GPU pose-graph refinement with a line process and edge pruning (csrc/posegraph.hip mvr_posegraph_optimize_lp,
lib.multiview.optimize_pose_graph(line_process=True)) against the numpy oracle (tests/posegraph_lp_oracle.py) on its
seeded outlier scenes (posegraph_lp_oracle.cases()), and against the plain entry where no edge is uncertain.

iters, status, member, the accept / reject pattern and the pruned edges: exactly (test_posegraph_lp_host.py asserts
that no decision of any case is within 1e-6 of its threshold and that every l is at least 0.1 from the pruning
threshold).  Poses, costs and l: the rule of test_gpu_posegraph.py, per pass: 100 x the difference between the
oracle's runs with np.linalg.cholesky and np.linalg.solve (poses and l absolute, costs relative to the pass's initial
cost), for the costs 100 x the larger of that and the held cost's evaluation floor
(posegraph_lp_oracle.cost_evaluation_floor at the pass's first and last poses and l), 1e-12 where a floor is zero.
mu: 1e-12 relative."""
import functools

import numpy as np
import pytest

import posegraph_lp_oracle as LP
import posegraph_oracle as PO

pytestmark = pytest.mark.gpu

KEYS = ("R0", "t0", "R_pair", "t_pair", "ij", "info", "w")


def _gpu(sc, passes, **kw):
    from lib.multiview import optimize_pose_graph
    return optimize_pose_graph(*(sc[k] for k in KEYS), return_trace=True, line_process=True,
                               uncertain=sc.get("uncertain"), prune_passes=passes, **LP.GLOBAL, **kw)


def _pattern(trace, iters):
    return [bool(trace[k + 1] < trace[k]) for k in range(iters)]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """-> the driver's dict and per pass (pose bound, cost bound, line bound)"""
    sc, _, kw, _ = LP.cases()[name]
    a, b = LP.run_case(name), LP.run_case(name, solver="solve")
    bounds = []
    w = sc["w"].copy()
    start = (sc["R0"], sc["t0"])
    for pa, pb in zip(a["passes"], b["passes"]):
        assert pa["accepted"] == pb["accepted"] and pa["status"] == pb["status"], name
        assert np.array_equal(pa["line"] < 0.25, pb["line"] < 0.25)
        c0 = max(pa["cost"][0], 1e-300)
        f_pose = max(np.abs(pa["R"] - pb["R"]).max(), np.abs(pa["t"] - pb["t"]).max())
        f_line = np.abs(pa["line"] - pb["line"]).max()
        f_cost = np.abs(pa["trace"] - pb["trace"]).max() / c0
        scp = dict(sc, w=w)
        first = LP.optimize(*start, sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], w, sc.get("uncertain"),
                            LP.MU_SCALE, **dict(kw, max_iters=0))
        f_eval = max(LP.cost_evaluation_floor(scp, *start, np.where(first["counted"], first["line"], 1.0), pa["mu"]),
                     LP.cost_evaluation_floor(scp, pa["R"], pa["t"], np.where(pa["counted"], pa["line"], 1.0),
                                              pa["mu"])) / c0
        f_cost = max(f_cost, f_eval)
        bounds.append(tuple(100.0 * f if f > 0 else 1e-12 for f in (f_pose, f_cost, f_line)))
        w = np.where(pa["counted"] & pa["uncertain"] & (pa["line"] < 0.25), 0.0, w)
        start = (pa["R"], pa["t"])
    return a, bounds


def _compare(name, k, got, want, bounds, sc, max_iters):
    tol_pose, tol_cost, tol_line = bounds
    n, it, c0 = len(sc["R0"]), want["iters"], max(want["cost"][0], 1e-300)
    d_pose = max(np.abs(got["R"] - want["R"]).max(), np.abs(got["t"] - want["t"]).max())
    d_cost = max(np.abs(got["trace"] - want["trace"]).max(), np.abs(got["cost"] - want["cost"]).max()) / c0
    print("%s pass %d: N %d, E %d, trials %d, status %d, cost %.6g -> %.6g, mu %.6g; |d pose| %.3g (bound %.3g), "
          "|d cost| / c0 %.3g (bound %.3g)" % (name, k, n, len(sc["ij"]), it, want["status"], want["cost"][0],
                                              want["cost"][1], want["mu"], d_pose, tol_pose, d_cost, tol_cost))
    assert int(got["iters"]) == it and int(got["status"]) == want["status"]
    np.testing.assert_array_equal(got["member"], want["member"])
    assert got["trace"].shape == (max_iters + 1,)
    assert (got["trace"][it + 1:] == -1.0).all() and (got["trace"][:it + 1] >= 0).all()
    assert _pattern(got["trace"], it) == want["accepted"] == _pattern(want["trace"], it)
    assert got["cost"][0] == got["trace"][0] and got["cost"][1] == got["trace"][it]
    assert d_pose <= tol_pose and d_cost <= tol_cost
    assert abs(float(got["mu"]) - want["mu"]) <= 1e-12 * want["mu"]
    return tol_line


@pytest.mark.parametrize("name", sorted(LP.cases()))
def test_matches_oracle(gpu, name):
    sc, _, kw, passes = LP.cases()[name]
    want, bounds = _oracle(name)
    got = _gpu(sc, passes, **kw)
    last = len(want["passes"]) - 1
    tol_line = _compare(name, last, got, want["passes"][last], bounds[last], sc, kw["max_iters"])
    assert len(got["passes"]) == last + 1
    for k, (gp, wp) in enumerate(zip(got["passes"], want["passes"])):
        assert int(gp["iters"]) == wp["iters"] and int(gp["status"]) == wp["status"]
        assert np.abs(gp["cost"] - wp["cost"]).max() <= bounds[k][1] * max(wp["cost"][0], 1e-300)
    if last:     # the first pass on its own: its trace and its l
        one = _gpu(sc, 1, **kw)
        first = want["passes"][0]
        t1 = _compare(name, 0, one, first, bounds[0], sc, kw["max_iters"])
        d = np.abs(one["line"] - first["line"]).max()
        print("%s pass 0: |d l| %.3g (bound %.3g)" % (name, d, t1))
        assert d <= t1 and np.array_equal(~one["kept"], first["uncertain"] & (first["line"] < 0.25))
    d = np.abs(got["line"] - want["line"]).max()
    print("%s: |d l| %.3g (bound %.3g), %d pruned" % (name, d, max(tol_line, bounds[0][2]), (~want["kept"]).sum()))
    assert d <= max(tol_line, bounds[0][2])
    assert got["kept"].dtype == bool and np.array_equal(got["kept"], want["kept"])
    held = [f for f in range(len(sc["R0"])) if not want["member"][f] or f == 0]
    assert got["R"][held].tobytes() == sc["R0"][held].tobytes() and got["t"][held].tobytes() == sc["t0"][held].tobytes()


@pytest.mark.parametrize("name,kw", [("bad_edges", PO.TWO), ("n30_noisy", dict(PO.TWO, max_iters=3)),
                                     ("reject", dict(PO.TWO, max_iters=8))])
def test_no_uncertain_edge_is_the_plain_entry_byte_for_byte(gpu, name, kw):
    from lib.multiview import optimize_pose_graph
    sc = PO.cases()[name][0]
    plain = optimize_pose_graph(*(sc[k] for k in KEYS), return_trace=True, **kw)
    got = _gpu(dict(sc, uncertain=np.zeros(len(sc["ij"]), np.int32)), 0, **kw)
    assert int(got["iters"]) == kw["max_iters"]
    for key in plain:
        assert np.asarray(got[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    wc, _, _ = PO.edge_weights(len(sc["R0"]), 0, sc["R_pair"], sc["t_pair"], sc["ij"], sc["w"], sc["info"])
    assert np.array_equal(got["line"], (wc > 0).astype(np.float64)) and float(got["mu"]) == 0.0 and got["kept"].all()


def test_a_scene_alone_and_in_a_ragged_batch(gpu):
    from lib.multiview import optimize_pose_graph
    C = LP.cases()
    kw = dict(C["out30"][2], return_trace=True, line_process=True, **LP.GLOBAL)
    main = C["out30"][0]
    alone = optimize_pose_graph(*(main[k] for k in KEYS), **kw)
    assert (~alone["kept"]).sum() == C["out30"][1].sum()
    scs = [C["out6"][0], main, C["bad_edges"][0]]
    for unc in (None, [np.ones(len(s["ij"]), np.int32) for s in scs]):       # NULL and all ones: the same edges
        out = optimize_pose_graph(*([s[k] for s in scs] for k in KEYS), uncertain=unc, **kw)
        assert out["R"].shape == (3, 30, 3, 3) and out["line"].shape == (3, 435) and out["mu"].shape == (3,)
        for key in ("R", "t", "member"):
            assert np.ascontiguousarray(out[key][1, :30]).tobytes() == alone[key].tobytes(), key
        for key in ("cost", "iters", "status", "trace", "line", "kept", "mu"):
            assert np.ascontiguousarray(out[key][1]).tobytes() == alone[key].tobytes(), key
        for k in range(2):
            for key in ("iters", "status", "cost"):
                assert np.ascontiguousarray(out["passes"][k][key][1]).tobytes() == alone["passes"][k][key].tobytes()
        assert not out["line"][0, len(scs[0]["ij"]):].any() and out["kept"][0, len(scs[0]["ij"]):].all()


def test_degenerate_scenes(gpu):
    from lib.multiview import PG_STATUS_LINE_PROCESS_OFF, optimize_pose_graph
    sc = LP.cases()["out6"][0]
    # the uncertain edges all have weight 0: none counts, mu 0, no bit, the plain entry's bytes
    flag = (sc["ij"][:, 1] != sc["ij"][:, 0] + 1)
    none = dict(sc, w=np.where(flag, 0.0, sc["w"]), uncertain=flag.astype(np.int32))
    got = _gpu(none, 0, **LP.TRIALS)
    plain = optimize_pose_graph(*(none[k] for k in KEYS), return_trace=True, **LP.TRIALS)
    assert int(got["status"]) == 0 and float(got["mu"]) == 0.0 and got["kept"].all()
    assert np.array_equal(got["line"], (~flag).astype(np.float64))                       # 1 on the chain, 0 elsewhere
    for key in plain:
        assert np.asarray(got[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    # zero information on the uncertain edges: bit 16, l = 1, the plain entry's poses
    zero = LP.zero_information_scene()
    want = LP.run(zero, mu_scale=LP.MU_SCALE, **LP.TRIALS)
    got = _gpu(zero, 0, **LP.TRIALS)
    plain = optimize_pose_graph(*(zero[k] for k in KEYS), return_trace=True, **LP.TRIALS)
    assert int(got["status"]) == want["status"] == PG_STATUS_LINE_PROCESS_OFF and float(got["mu"]) == 0.0
    assert (got["line"] == 1.0).all() and got["kept"].all()
    for key in ("R", "t", "member", "cost", "iters", "trace"):
        assert np.asarray(got[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    # an invalid scene in a batch: poses copied through, l 0
    bad = dict(sc, t0=sc["t0"].copy())
    bad["t0"][2, 1] = np.nan
    out = optimize_pose_graph(*([s[k] for s in (sc, bad)] for k in KEYS), return_trace=True, line_process=True,
                              **LP.GLOBAL, **LP.TRIALS)
    assert out["status"].tolist() == [0, 5] and not out["line"][1].any() and not out["member"][1].any()
    assert out["R"][1].tobytes() == bad["R0"].tobytes() and out["t"][1].tobytes() == bad["t0"].tobytes()
    assert out["mu"][1] == 0.0 and (out["trace"][1] == -1.0).all() and out["kept"][1].all()


def test_abi_rejects_a_bad_mu_scale(gpu):
    import torch
    from lib import _native as N
    L = N.lib()
    sc = LP.cases()["out6"][0]
    E, n = len(sc["ij"]), len(sc["R0"])
    d = {k: torch.from_numpy(np.ascontiguousarray(sc[k].astype(np.int32) if k == "ij" else sc[k])).to(gpu)
         for k in KEYS}
    R, t = torch.full((n, 9), 7.0, dtype=torch.float64, device=gpu), torch.zeros(n, 3, dtype=torch.float64, device=gpu)
    cost, line = torch.zeros(2, dtype=torch.float64, device=gpu), torch.zeros(E, dtype=torch.float64, device=gpu)
    cnt = torch.tensor([E, n], dtype=torch.int32, device=gpu)
    ints = torch.zeros(2, dtype=torch.int32, device=gpu)
    ws = torch.empty(L.mvr_posegraph_lp_workspace_bytes(1, n, E), dtype=torch.uint8, device=gpu)

    def call(mu_scale):
        return L.mvr_posegraph_optimize_lp(
            N.ptr(d["R_pair"]), N.ptr(d["t_pair"]), N.ptr(d["ij"]), N.ptr(d["w"]), N.ptr(d["info"]), None, E,
            N.ptr(cnt[:1]), N.ptr(cnt[1:]), 1, n, E, 0, N.ptr(d["R0"]), N.ptr(d["t0"]), 2, 1e-6, 0.0, 0.0, mu_scale,
            N.ptr(R), N.ptr(t), n, None, N.ptr(cost), N.ptr(ints[:1]), N.ptr(ints[1:]), None, N.ptr(line), None,
            N.ptr(ws), ws.numel(), N.stream())
    for mu_scale in (0.0, -0.0025, float("inf"), float("nan")):
        assert call(mu_scale) == -1
    torch.cuda.synchronize()
    assert (R == 7.0).all()                                # nothing was launched
    assert call(LP.MU_SCALE) == 0
    torch.cuda.synchronize()
    assert int(ints[0]) == 2 and not (R == 7.0).any()


@pytest.mark.parametrize("name", ["out8", "out30"])
def test_quality_and_python_surface(gpu, name):
    """default tolerances, two passes: prunes exactly the planted edges, ends within 0.05 rad / 0.05 m of the ground
    truth (the oracle: at most 0.021 / 0.021) where the plain call ends above 0.4 rad"""
    import torch
    from lib.multiview import optimize_pose_graph
    sc, bad, _, _ = LP.cases()[name]
    args = tuple(torch.from_numpy(sc[k]).to(gpu) for k in KEYS)
    plain = optimize_pose_graph(*args)
    got = optimize_pose_graph(*args, line_process=True, **LP.GLOBAL)
    assert set(got) == set(plain) | {"line", "kept", "mu", "passes"} and len(got["passes"]) == 2
    assert all(torch.is_tensor(v) and v.device.type == "cuda" for k, v in got.items() if k != "passes")
    assert all(set(p) == {"iters", "status", "cost"} and p["cost"].shape == (2,) for p in got["passes"])
    assert got["kept"].dtype == torch.bool and got["line"].shape == (len(bad),) and got["mu"].shape == ()
    e0 = PO.pose_error(plain["R"].cpu().numpy(), plain["t"].cpu().numpy(), sc["R_gt"], sc["t_gt"])
    e1 = PO.pose_error(got["R"].cpu().numpy(), got["t"].cpu().numpy(), sc["R_gt"], sc["t_gt"])
    line = got["line"].cpu().numpy()
    print("%s: plain %.3g rad / %.3g m, line process %.4g rad / %.4g m; %d pruned, largest l of an outlier %.3g, "
          "smallest of another edge %.3g, trials %s" % ((name,) + e0 + e1 + (
              bad.sum(), line[bad].max(), line[~bad].min(), [int(p["iters"]) for p in got["passes"]])))
    assert np.array_equal(~got["kept"].cpu().numpy(), bad)
    assert e1[0] <= 0.05 and e1[1] <= 0.05 and e0[0] > 0.4 and e1[0] < e0[0] and e1[1] < e0[1]
    # prune_passes 0: one optimisation, nothing pruned; numpy in, numpy out
    one = optimize_pose_graph(*(sc[k] for k in KEYS), line_process=True, prune_passes=0, **LP.GLOBAL)
    assert isinstance(one["line"], np.ndarray) and one["kept"].all() and len(one["passes"]) == 1
    assert np.array_equal(one["line"] < 0.25, bad)


def test_pruning_that_disconnects_the_graph(gpu):
    sc, bad = LP.disconnecting_scene()
    want = LP.global_optimization(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"], None,
                                  LP.MU_SCALE, **LP.TRIALS)
    got = _gpu(sc, 2, **LP.TRIALS)
    assert [int(p["status"]) for p in got["passes"]] == [p["status"] for p in want["passes"]] == [0, 1]
    assert got["member"].tolist() == [1] * 7 + [0] and np.array_equal(~got["kept"], bad)
    first = _gpu(sc, 1, **LP.TRIALS)
    assert got["R"][7].tobytes() == first["R"][7].tobytes() and got["t"][7].tobytes() == first["t"][7].tobytes()
    np.testing.assert_allclose(got["R"], want["R"], rtol=0, atol=1e-9)
    assert (got["line"][bad] < 0.15).all() and (got["line"][~bad] > 0.35).all()


def test_register_scene_end_to_end(gpu):
    import icp_oracle as O
    from lib.multiview import register_scene
    raw = O.scene4()[0]
    init = O.scene4_starts(O.SIX, O.scene4_centroids())
    base = register_scene(raw, 0.025, init=init, min_frags=2)
    off = register_scene(raw, 0.025, init=init, min_frags=2, line_process=False, preference_loop_closure=3.0)
    assert "pruned" not in base["pairs"] and set(off["refined"]) == set(base["refined"])
    for key in ("R", "t", "member"):
        assert off[key].tobytes() == base[key].tobytes(), key
    assert off["scene"]["xyz"].cpu().numpy().tobytes() == base["scene"]["xyz"].cpu().numpy().tobytes()
    res = register_scene(raw, 0.025, init=init, min_frags=2, line_process=True)
    rec, ref = res["pairs"], res["refined"]
    print("register_scene(line_process): kept %s, pruned %s, l %s, mu %.6g, cost %.6g -> %.6g" % (
        rec["kept"].astype(int), rec["pruned"].astype(int), np.round(ref["line"], 3), float(ref["mu"]),
        ref["cost"][0], ref["cost"][1]))
    assert np.isfinite(res["poses"]).all() and rec["pruned"].dtype == bool and rec["pruned"].shape == (6,)
    assert not (rec["pruned"] & ~rec["kept"]).any() and rec["pruned"][rec["kept"]].tolist() == (~ref["kept"]).tolist()
    assert len(ref["passes"]) == 2 and float(ref["mu"]) > 0 and len(res["scene"]["xyz"]) > 0
    assert res["member"][0] == 1 and np.isfinite(res["scene"]["xyz"].cpu().numpy()).all()
