"""Host-side checks of the pose-graph refinement's oracle (tests/posegraph_oracle.py), of the scenes
test_gpu_posegraph.py runs, and of the argument rules of lib.multiview.optimize_pose_graph and
mvr_posegraph_optimize.  No GPU.

The scenes are generated from seeded RNGs (posegraph_oracle.scene; every case of posegraph_oracle.cases() uses
seed 1): fragments of random poses, edges all pairs or a ring plus chords, T_k exact or off by 1 degree / 1 cm,
info_k from the information oracle on 40 random points per edge, weights with zeros."""
import functools

import numpy as np
import pytest

import posegraph_oracle as PO


@functools.lru_cache(maxsize=None)
def _exact(n, edges):
    sc = PO.scene(n, 1, edges)
    return sc, PO.run(sc)


@functools.lru_cache(maxsize=None)
def _noisy(n, edges):
    sc = PO.scene(n, 1, edges, True, min(3, n // 3))     # some chords with weight 0
    return sc, PO.run(sc)


@pytest.mark.parametrize("n,edges", [(3, "all"), (30, "all"), (64, "ring")])
def test_exact_edges_return_the_ground_truth(n, edges):
    """Starts 3 degrees / 5 cm off, default settings.  Measured before the bound was fixed (rotation angle in rad,
    translation in m): 3 fragments 1.2e-16 / 1.1e-15, 30 fragments 8.9e-17 / 1.1e-15, 64 fragments 4.7e-16 / 2.3e-15.
    The bound is 100 x the largest: 4.7e-14 rad, 2.3e-13 m."""
    sc, out = _exact(n, edges)
    er, et = PO.pose_error(out["R"], out["t"], sc["R_gt"], sc["t_gt"])
    e0 = PO.pose_error(sc["R0"], sc["t0"], sc["R_gt"], sc["t_gt"])
    print("%d fragments: start %.3g rad / %.3g m, end %.3g rad / %.3g m, %d trials"
          % ((n,) + e0 + (er, et, out["iters"])))
    assert abs(e0[0] - np.deg2rad(3.0)) < 1e-9 and abs(e0[1] - 0.05) < 1e-9
    assert out["status"] == 0 and out["member"].all() and out["iters"] < 20
    assert er <= 4.7e-14 and et <= 2.3e-13
    assert out["cost"][1] <= 1e-24 * out["cost"][0]


@pytest.mark.parametrize("n,edges", [(3, "all"), (30, "all"), (43, "ring"), (64, "ring")])
def test_noisy_scenes_reach_a_stationary_point(n, edges):
    sc, out = _noisy(n, edges)
    k = out["iters"]
    tr = out["trace"]
    assert out["status"] == 0 and (tr[:k + 1] >= 0).all() and (tr[k + 1:] == -1.0).all()
    assert (np.diff(tr[:k + 1]) <= 0).all()                      # the held cost never rises
    for i, acc in enumerate(out["accepted"]):                    # strictly lower on an accepted trial, equal otherwise
        assert (tr[i + 1] < tr[i]) if acc else (tr[i + 1] == tr[i])
    assert out["cost"][0] == tr[0] and out["cost"][1] == tr[k]
    args = (sc["R_pair"], sc["t_pair"], sc["ij"], sc["w"], sc["info"])
    g0 = PO.gradient_norm(sc["R0"], sc["t0"], *args)
    g1 = PO.gradient_norm(out["R"], out["t"], *args)
    print("%d fragments: cost %.6g -> %.6g in %d trials, |g| %.3g -> %.3g" % (n, tr[0], tr[k], k, g0, g1))
    assert g1 <= 1e-8 * g0
    # and it is no worse than the ground truth, which the noise has moved the minimum away from
    assert out["cost"][1] <= PO.cost(sc["R_gt"], sc["t_gt"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["w"],
                                     sc["info"]) * (1 + 1e-12)


def test_jacobian_is_first_order():
    """g = the gradient of c / 2 by central differences of the cost over the left update"""
    sc = PO.scene(5, 1, "all", True, 1)
    R, t = sc["R0"], sc["t0"]
    args = (sc["R_pair"], sc["t_pair"], sc["ij"])
    wc, member, _ = PO.edge_weights(5, 0, *args, sc["w"], sc["info"])
    _, g = PO.system(R, t, *args, wc, sc["info"], member, 0)
    h = 1e-6
    for f in (1, 4):
        for q in range(6):
            c = []
            for sgn in (1.0, -1.0):
                d = np.zeros(6)
                d[q] = sgn * h
                Ex = PO.so3_exp(d[3:])
                R2, t2 = R.copy(), t.copy()
                R2[f], t2[f] = Ex @ R[f], Ex @ t[f] + d[:3]
                c.append(PO.cost(R2, t2, *args, wc, sc["info"]))
            num = (c[0] - c[1]) / (4 * h)
            # first order: xi is not small at the start (3 degrees), so J drops the terms of relative size |xi|
            assert abs(num - g[6 * f + q]) <= 0.1 * np.abs(g).max(), (f, q, num, g[6 * f + q])


def test_every_decision_of_every_gpu_case_clears_rounding():
    """accept margins (c - c') / c and stop margins (relative distance from the threshold) >= 1e-6 in every trial of
    every case test_gpu_posegraph.py compares with the kernel; all scenes from seed 1"""
    for name, (sc, kw) in PO.cases().items():
        out = PO.run(sc, **kw)
        m = np.asarray(out["margins"] + [(np.inf, np.inf)])
        print("%-20s trials %-9s accept margin %.3g, stop margin %.3g" % (
            name, "".join("F" if f else ("A" if a else "r") for a, f in zip(out["accepted"], out["failed"])),
            m[:, 0].min(), m[:, 1].min()))
        assert m.min() >= 1e-6, name


def test_case_statuses_are_what_their_names_say():
    res = {name: PO.run(sc, **kw) for name, (sc, kw) in PO.cases().items() if not name.startswith("n128")}
    assert res["n1"]["iters"] == 0 and res["n1"]["status"] == 0 and res["n1"]["member"].tolist() == [1]
    assert res["edges_0"]["status"] == 1 and res["edges_0"]["member"].sum() == 1 and res["edges_0"]["iters"] == 0
    assert res["edges_1"]["status"] == 1 and res["edges_1"]["member"].sum() == 2
    assert all(res["edges_%d" % E]["status"] == 0 for E in PO.EDGE_COUNTS[2:])
    assert res["n30_noisy"]["iters"] == 2 and res["n30_noisy"]["status"] == 0          # tolerances 0: max_iters trials
    assert res["reject"]["iters"] == 8 and res["reject"]["accepted"] == [False] * 4 + [True] * 4
    assert res["n30_noisy_tol"]["iters"] == 2 and res["n30_noisy_tol"]["status"] == 0   # stopped by tol_cost
    assert res["n30_noisy_cap"]["iters"] == 1 and res["n30_noisy_cap"]["status"] == 2
    assert all(res["n%d_exact" % n]["iters"] == 3 and res["n%d_exact" % n]["status"] == 0 for n in (2, 3, 30, 43, 64))
    bad = res["bad_edges"]
    sc = PO.cases()["bad_edges"][0]
    wc, _, ignored = PO.edge_weights(8, 0, sc["R_pair"], sc["t_pair"], sc["ij"], sc["w"], sc["info"])
    assert bad["status"] == 4 and ignored and (wc[-PO.N_IGNORED - 1:-1] == 0).all() and wc[-1] > 0 and wc[2] == 0
    assert wc[28] > 0 and wc[29] > 0                                                    # repeated and (j, i): count
    d = res["disconnected"]
    assert d["status"] == 1 and d["member"].tolist() == [1] * 6 + [0] * 3
    sc = PO.cases()["disconnected"][0]
    assert d["R"][6:].tobytes() == sc["R0"][6:].tobytes() and d["t"][6:].tobytes() == sc["t0"][6:].tobytes()
    a3 = res["anchor3"]
    sc = PO.cases()["anchor3"][0]
    assert a3["R"][3].tobytes() == sc["R0"][3].tobytes() and a3["t"][3].tobytes() == sc["t0"][3].tobytes()
    assert not np.array_equal(a3["R"][0], sc["R0"][0]) or not np.array_equal(a3["t"][0], sc["t0"][0])
    assert res["zero_info"]["status"] == 0
    z = res["zero_info_only_edge"]                    # the fragment's block of H is exactly zero: pivot 0, every trial
    assert z["failed"] == [True] * 4 and z["status"] == (2 | 8) and z["cost"][0] == z["cost"][1]
    assert PO.run(PO.cases()["zero_info_only_edge"][0], max_iters=4, solver="solve")["failed"] == [True] * 4
    # the edge test decides the component: the ignored edge was the only way to fragment 2
    cut = res["cut_by_bad_edge"]
    assert cut["status"] == 5 and cut["member"].tolist() == [1, 1, 0] and cut["accepted"] == [True, True]
    assert min(m[0] for m in cut["margins"]) >= 0.999
    one = res["n1_bad_edges"]
    assert one["status"] == 4 and one["member"].tolist() == [1] and one["iters"] == 0 and not one["cost"].any()
    # invalid scenes
    sc = PO.cases()["n3_noisy"][0]
    inv = PO.run(sc, anchor=3)
    assert inv["status"] == 5 and not inv["member"].any() and inv["R"].tobytes() == sc["R0"].tobytes()
    sc2 = dict(sc, t0=sc["t0"].copy())
    sc2["t0"][2, 1] = np.nan
    assert PO.run(sc2)["status"] == 5


def _scene_args(sc):
    return (sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"])


def test_wrapper_argument_rules_without_a_device():
    from lib.multiview import optimize_pose_graph
    sc = PO.scene(4, 1, "all", True)
    a = _scene_args(sc)
    for kw, msg in ((dict(max_iters=-1), "max_iters"), (dict(lambda0=-1.0), "lambda0"),
                    (dict(lambda0=float("inf")), "lambda0"), (dict(lambda0=float("nan")), "lambda0"),
                    (dict(tol_cost=-1e-9), "tolerances"), (dict(tol_step=float("nan")), "tolerances"),
                    (dict(anchor=4), "anchor"), (dict(anchor=-1), "anchor")):
        with pytest.raises(ValueError, match=msg):
            optimize_pose_graph(*a, **kw)
    with pytest.raises(ValueError, match="R must be"):
        optimize_pose_graph(sc["R0"].reshape(-1, 9), *a[1:])
    with pytest.raises(ValueError, match="R_pair must be"):
        optimize_pose_graph(a[0], a[1], sc["R_pair"][None], *a[3:])
    with pytest.raises(ValueError, match="one per edge"):
        optimize_pose_graph(*a[:5], sc["info"][:-1])
    with pytest.raises(ValueError, match="one per edge"):
        optimize_pose_graph(*a, weights=np.ones(3))
    with pytest.raises(ValueError, match="one row per pose"):
        optimize_pose_graph(a[0], sc["t0"][:-1], *a[2:])
    with pytest.raises(ValueError, match="at most"):
        optimize_pose_graph(np.tile(np.eye(3), (129, 1, 1)), np.zeros((129, 3)), *a[2:])
    with pytest.raises(ValueError, match="per-scene lists"):
        optimize_pose_graph([a[0]], [a[1]], [a[2]], [a[3]], [a[4]], [a[5], a[5]])
    with pytest.raises(ValueError, match="n_frags"):
        optimize_pose_graph(*(x[None] for x in a), n_frags=[5])
    with pytest.raises(ValueError, match="n_edges"):
        optimize_pose_graph(*(x[None] for x in a), n_edges=[7])


def test_abi_argument_rules_without_a_device():
    from lib import _native as N
    L = N.lib()
    Z = None

    def call(S=0, F=0, E=0, anchor=0, iters=5, lam=1e-6, tc=0.0, ts=0.0, ws=0, ptr=Z):
        return L.mvr_posegraph_optimize(ptr, ptr, ptr, Z, ptr, E, ptr, ptr, S, F, E, anchor, ptr, ptr, iters, lam, tc,
                                        ts, ptr, ptr, F, Z, ptr, ptr, ptr, Z, ptr, ws, Z)

    assert call() == 0 and call(S=0, F=30, E=435) == 0              # S = 0: NULL pointers
    assert call(S=4, F=0, E=0) == 0                                 # F = 0: nothing to write
    assert call(S=1, F=3, E=3) == -1                                # work to do, NULL pointers
    for kw in (dict(S=-1), dict(F=-1), dict(E=-1), dict(F=129), dict(F=3, anchor=3), dict(anchor=-1), dict(iters=-1),
               dict(lam=-1.0), dict(lam=float("inf")), dict(lam=float("nan")), dict(tc=-1.0), dict(ts=float("nan"))):
        assert call(**kw) == -1, kw
    assert L.mvr_posegraph_workspace_bytes(0, 30, 435) == 0
    assert L.mvr_posegraph_workspace_bytes(1, 30, 435) == 8 * (43 * 435 + 181 * 180)
    assert L.mvr_posegraph_workspace_bytes(3, 128, 0) == 3 * 8 * 769 * 768
    # a workspace one byte short: rejected before anything is launched (the pointers are never followed)
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = L.mvr_posegraph_workspace_bytes(1, 3, 3)
    assert call(S=1, F=3, E=3, ws=need - 1, ptr=p) == -1
    assert call(S=1, F=3, E=3, ws=need, ptr=ctypes.c_void_p(p.value + 4)) == -1      # misaligned
