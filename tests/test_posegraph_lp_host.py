"""Host-side checks of the line-process oracle (tests/posegraph_lp_oracle.py), of the scenes
test_gpu_posegraph_lp.py runs, and of the argument rules of lib.multiview.optimize_pose_graph(line_process=True) and
mvr_posegraph_optimize_lp.  No GPU.

The scenes are posegraph_oracle.scene's noisy all-pairs scenes (starts 3 degrees / 5 cm off) with a share of the edges
j != i + 1 replaced by random transforms (posegraph_lp_oracle.with_outliers, seed = the scene's + 100);
mu_scale = 0.0025 (preference_loop_closure 1, max_correspondence_distance 0.05), every edge uncertain unless the case
says otherwise."""
import functools
import os
import re

import numpy as np
import pytest

import posegraph_lp_oracle as LP
import posegraph_oracle as PO

THRESHOLD = 0.25


@functools.lru_cache(maxsize=None)
def _case(name):
    return LP.run_case(name)


@pytest.mark.parametrize("name", ["n3_noisy", "n30_noisy_tol", "reject", "bad_edges", "disconnected", "anchor3",
                                  "zero_info_only_edge", "n1", "edges_1"])
def test_all_edges_certain_is_the_plain_oracle(name):
    """uncertain all zero: every number posegraph_oracle.optimize returns, bit for bit"""
    sc, kw = PO.cases()[name]
    want = PO.run(sc, **kw)
    got = LP.optimize(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"],
                      np.zeros(len(sc["ij"]), np.int32), LP.MU_SCALE, **kw)
    for key in ("R", "t", "member", "cost", "trace"):
        assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
    for key in ("iters", "status", "accepted", "failed", "margins"):
        assert got[key] == want[key], key
    assert got["mu"] == 0.0 and not got["uncertain"].any()
    assert np.array_equal(got["line"], got["counted"].astype(np.float64))


@pytest.mark.parametrize("name", ["out6", "out8", "long", "reject", "chain_certain"])
def test_trace_falls_and_is_the_geman_mcclure_cost(name):
    sc, _, kw, _ = LP.cases()[name]
    out = LP.run(sc, mu_scale=LP.MU_SCALE, **kw)
    k, tr = out["iters"], out["trace"]
    assert (np.diff(tr[:k + 1]) <= 0).all() and (tr[k + 1:] == -1.0).all()
    for i, acc in enumerate(out["accepted"]):
        assert (tr[i + 1] < tr[i]) if acc else (tr[i + 1] == tr[i])
    # the held cost is formed from l; the closed form says it is sum_certain r + sum_uncertain mu r / (mu + r)
    gm = LP.geman_mcclure(out["r"], out["mu"], out["counted"], out["uncertain"])
    print("%s: cost %.9g -> %.9g, Geman-McClure %.9g, %d uncertain of %d counted"
          % (name, tr[0], tr[k], gm, out["uncertain"].sum(), out["counted"].sum()))
    assert abs(out["cost"][1] - gm) <= 1e-13 * gm * out["counted"].sum()
    l, u = out["line"], out["uncertain"]
    assert (l[out["counted"] & ~u] == 1.0).all() and (l[~out["counted"]] == 0.0).all()
    np.testing.assert_allclose(l[u], (out["mu"] / (out["mu"] + out["r"][u])) ** 2, rtol=1e-15)


def test_line_process_recovers_what_the_plain_loop_cannot():
    """the issue's table, default tolerances: (rad / m) plain above 0.4, line process and pruning at most 0.021"""
    for n, seed, share in ((6, 1, 0.3), (8, 1, 0.3), (8, 2, 0.4), (12, 3, 0.4)):
        sc, bad = LP.outlier_scene(n, seed, share)
        plain = PO.run(sc)
        g = LP.global_optimization(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"], None,
                                   LP.MU_SCALE)
        e0 = PO.pose_error(plain["R"], plain["t"], sc["R_gt"], sc["t_gt"])
        e1 = PO.pose_error(g["R"], g["t"], sc["R_gt"], sc["t_gt"])
        print("%d fragments, seed %d, %d of %d edges outliers: plain %.3g / %.3g, line process %.4g / %.4g; largest l "
              "of an outlier %.3g, smallest of another edge %.3g" % ((n, seed, bad.sum(), len(bad)) + e0 + e1 + (
                  g["line"][bad].max(), g["line"][~bad].min())))
        assert e0[0] > 0.4 and max(e1) <= 0.021
        assert np.array_equal(~g["kept"], bad)


def test_every_decision_of_every_gpu_case_clears_rounding():
    """accept and stop margins >= 1e-6 in every trial of every pass of every case test_gpu_posegraph_lp.py compares
    with the kernel; and the pruning threshold is a condition, not a measurement: in every pass that prunes, every
    uncertain edge's l is at least 0.1 from it, and the pruned edges are exactly the planted outliers that count"""
    for name, (sc, bad, kw, prune_passes) in LP.cases().items():
        g = _case(name)
        for k, p in enumerate(g["passes"]):
            m = np.asarray(p["margins"] + [(np.inf, np.inf)])
            u = p["uncertain"]
            gap = np.abs(p["line"][u] - THRESHOLD).min()
            print("%-14s pass %d trials %-9s accept margin %.3g, stop margin %.3g, min |l - threshold| %.3g" % (
                name, k, "".join("F" if f else ("A" if a else "r") for a, f in zip(p["accepted"], p["failed"])),
                m[:, 0].min(), m[:, 1].min(), gap))
            assert m.min() >= 1e-6, name
            if prune_passes:
                assert gap >= 0.1, name
        if prune_passes:
            first = g["passes"][0]
            assert np.array_equal(~g["kept"], bad & first["uncertain"]), name
    assert _case("reject")["passes"][0]["accepted"] == [False] * 4 + [True] * 4
    assert _case("bad_edges")["status"] == 4 and _case("chain_certain")["passes"][0]["uncertain"].sum() == 21


def test_pruning_can_disconnect_a_fragment():
    sc, bad = LP.disconnecting_scene()
    g = LP.global_optimization(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"], None,
                               LP.MU_SCALE, **LP.TRIALS)
    assert [p["status"] for p in g["passes"]] == [0, 1]
    assert g["member"].tolist() == [1] * 7 + [0] and np.array_equal(~g["kept"], bad)
    for p in g["passes"]:
        assert np.asarray(p["margins"]).min() >= 1e-6
        assert np.abs(p["line"][p["uncertain"]] - THRESHOLD).min() >= 0.1
    # a fragment's only edge, however wrong, is met by moving the fragment: l goes to 1 and the edge stays
    sc, bad = LP.disconnecting_scene(links=(6,))
    g = LP.global_optimization(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"], None,
                               LP.MU_SCALE, **LP.TRIALS)
    assert [p["status"] for p in g["passes"]] == [0, 0] and g["member"].all()
    assert bad[-1] and g["kept"][-1] and g["line"][-1] > 0.9 and np.array_equal(~g["kept"][:-1], bad[:-1])


def test_mu_not_positive_switches_the_line_process_off():
    zero = LP.zero_information_scene()
    out = LP.run(zero, mu_scale=LP.MU_SCALE, **LP.TRIALS)
    assert out["status"] == LP.LINE_PROCESS_OFF and out["mu"] == 0.0 and not out["uncertain"].any()
    assert (out["line"] == 1.0).all()
    plain = PO.run(zero, **LP.TRIALS)
    assert out["R"].tobytes() == plain["R"].tobytes() and out["trace"].tobytes() == plain["trace"].tobytes()


def _scene_args(sc):
    return (sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"])


def test_wrapper_argument_rules_without_a_device():
    from lib import multiview
    from lib.multiview import optimize_pose_graph
    assert multiview.PG_STATUS_LINE_PROCESS_OFF == 16
    sc = PO.scene(4, 1, "all", True)
    a = _scene_args(sc)
    ok = dict(line_process=True, max_correspondence_distance=0.05)
    with pytest.raises(ValueError, match="max_correspondence_distance"):
        optimize_pose_graph(*a, line_process=True)
    for kw, msg in ((dict(max_correspondence_distance=0.0), "finite and positive"),
                    (dict(max_correspondence_distance=float("nan")), "finite and positive"),
                    (dict(preference_loop_closure=-1.0), "finite and positive"),
                    (dict(preference_loop_closure=float("inf")), "finite and positive"),
                    (dict(edge_prune_threshold=1.5), "edge_prune_threshold"),
                    (dict(edge_prune_threshold=float("nan")), "edge_prune_threshold"),
                    (dict(prune_passes=-1), "prune_passes"), (dict(max_iters=-1), "max_iters")):
        with pytest.raises(ValueError, match=msg):
            optimize_pose_graph(*a, **dict(ok, **kw))
    with pytest.raises(ValueError, match="one per edge"):
        optimize_pose_graph(*a, uncertain=np.ones(5, np.int32), **ok)
    with pytest.raises(ValueError, match="per-scene lists"):
        optimize_pose_graph(*([x] for x in a), uncertain=[np.ones(6), np.ones(6)], **ok)
    with pytest.raises(ValueError, match="one uncertain flag per edge"):
        optimize_pose_graph(*([x] for x in a), uncertain=[np.ones(5)], **ok)


def test_abi_argument_rules_without_a_device():
    import ctypes
    from lib import _native as N
    L = N.lib()
    Z = None

    def call(S=0, F=0, E=0, anchor=0, iters=5, lam=1e-6, tc=0.0, ts=0.0, mu=0.0025, ws=0, ptr=Z, line="ptr"):
        return L.mvr_posegraph_optimize_lp(ptr, ptr, ptr, Z, ptr, Z, E, ptr, ptr, S, F, E, anchor, ptr, ptr, iters,
                                           lam, tc, ts, mu, ptr, ptr, F, Z, ptr, ptr, ptr, Z,
                                           ptr if line == "ptr" else line, Z, ptr, ws, Z)

    assert call() == 0 and call(S=0, F=30, E=435) == 0 and call(S=4, F=0, E=0) == 0
    assert call(S=1, F=3, E=3) == -1
    for kw in (dict(mu=0.0), dict(mu=-1.0), dict(mu=float("inf")), dict(mu=float("nan")), dict(S=-1), dict(F=129),
               dict(F=3, anchor=3), dict(iters=-1), dict(lam=float("nan")), dict(tc=-1.0)):
        assert call(**kw) == -1, kw
    assert L.mvr_posegraph_lp_workspace_bytes(0, 30, 435) == 0
    assert L.mvr_posegraph_lp_workspace_bytes(1, 30, 435) == 8 * (45 * 435 + 181 * 180)
    assert L.mvr_posegraph_lp_workspace_bytes(3, 128, 0) == L.mvr_posegraph_workspace_bytes(3, 128, 0)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = L.mvr_posegraph_lp_workspace_bytes(1, 3, 3)
    assert call(S=1, F=3, E=3, ws=need - 1, ptr=p) == -1       # rejected before anything is launched
    assert call(S=1, F=3, E=3, ws=L.mvr_posegraph_workspace_bytes(1, 3, 3), ptr=p) == -1
    assert call(S=1, F=3, E=3, ws=need, ptr=p, line=Z) == -1   # a NULL line with edges


def test_header_declares_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mvreg.h")) as f:
        text = f.read()
    assert re.search(r"^size_t mvr_posegraph_lp_workspace_bytes\(int S, int max_frags, int max_edges\);", text, re.M)
    decl = re.search(r"^int mvr_posegraph_optimize_lp\(([^;]*)\);", text, re.M)
    assert decl and "const int32_t* uncertain" in decl.group(1) and "double mu_scale" in decl.group(1)
    assert "double* line" in decl.group(1) and "double* mu" in decl.group(1)
    assert "no line process or robust kernel)" not in text


def test_scripts_take_the_flags():
    from scripts import multiview_sync, register_scene
    a = register_scene.parser().parse_args(["--fragments", "a", "b", "--out", "o", "--line_process",
                                            "--preference_loop_closure", "2"])
    assert a.line_process and a.preference_loop_closure == 2.0
    assert not register_scene.parser().parse_args(["--fragments", "a", "b", "--out", "o"]).line_process
    with pytest.raises(SystemExit):      # --line_process without --line_max_dist, before any file is read
        multiview_sync.main(["--traj", "none", "--n_fragments", "3", "--out", "o", "--info", "none", "--refine",
                             "--line_process"])
