"""GPU robust kernels on the three ICP variants (csrc/icp_robust.hip mvr_icp_refine_robust, lib/icp.py kernel=) against
the plain entries (l2: bit for bit) and the numpy / sklearn oracle (tests/icp_robust_oracle.py): every method with
every kernel on the scene, small shapes and status bits, batch and translation invariance, what the kernels buy on a
contaminated pair, the Python surface and register_scene's icp_kernel.

Tolerance: 1e-9 on T, fitness, rmse and the trace (the project's fp64 bound), 1e-9 relative on w_sum; n_corr, iters
and status exactly.  The comparisons feed the oracle the GPU's own points and normals.  test_icp_robust_host.py checks
that no scene case used here has a correspondence or a stopping test within rounding of a tie."""
import functools
import os
import sys

import numpy as np
import pytest

import gicp_oracle as GO
import icp_oracle as O
import icp_plane_oracle as PO
import icp_robust_oracle as RO

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
if HELPERS not in sys.path:
    sys.path.insert(0, HELPERS)

pytestmark = pytest.mark.gpu
TOL = 1e-9
SENTINEL = -77.0
# A solve is compared with the oracle's where its rounding stays below TOL: the two differ by about eps cond per solve
# (2.2e-16 cond), so cond <= 1e5 leaves 2e-11 per solve and 30 solves of a contractive loop below 1e-9.  The pairs
# beyond (a target of one or two points, a flat target) are compared up to their first evaluation, which no solve enters
COND_MAX = 1e5
PLAIN = {"point_to_point": "mvr_icp_refine", "point_to_plane": "mvr_icp_refine_plane",
         "generalized": "mvr_icp_refine_generalized"}
NAMES = ("T", "fitness", "rmse", "n_corr", "iters", "status", "trace")


@functools.lru_cache(maxsize=None)
def _fo():
    """the scene's centroids on an index of cell 0.075, with normals over that radius"""
    from lib.overlap import FragmentOverlap
    fo = FragmentOverlap(O.scene4()[0], "FCGF", 0.025)
    fo.estimate_normals()
    return fo


def _split(fo, x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    return [x[fo.off[b]:fo.off[b + 1]] for b in range(fo.B)]


@functools.lru_cache(maxsize=None)
def _six_starts():
    return O.scene4_starts(O.SIX, O.scene4_centroids())


def _raw(fo, method, kernel, k, pairs, T0, max_dist, max_iters, tol, epsilon=GO.EPSILON, plain=False):
    """mvr_icp_refine_robust (plain: the method's own entry) on sentinel-filled output buffers -> numpy outputs"""
    import torch
    from lib import _native as N
    d = fo.device
    P = len(pairs)
    gp = torch.as_tensor(np.asarray(pairs, np.int64).reshape(-1, 2)).to(d)
    gT = torch.as_tensor(np.ascontiguousarray(np.asarray(T0, np.float64)[:, :3])).to(d)
    T = torch.full((P, 12), SENTINEL, dtype=torch.float64, device=d)
    fit, rm, ws = (torch.full((P,), SENTINEL, dtype=torch.float64, device=d) for _ in range(3))
    nc, it, st = (torch.full((P,), int(SENTINEL), dtype=torch.int32, device=d) for _ in range(3))
    tr = torch.full((P, max_iters + 1, 2), SENTINEL, dtype=torch.float64, device=d)
    nrm = () if plain and method == "point_to_point" else (N.ptr(fo.normals),)
    head = (N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz)) + nrm + (N.ptr(fo.off_dev), fo.B, fo.M, fo.r, N.ptr(gp),
                                                                       N.ptr(gT), P)
    outs = (N.ptr(T), N.ptr(fit), N.ptr(rm), N.ptr(nc), N.ptr(it), N.ptr(st), N.ptr(tr))
    if plain:
        eps = (epsilon,) if method == "generalized" else ()
        N.check(getattr(N.lib(), PLAIN[method])(*head, max_dist, *eps, max_iters, tol, tol, *outs, N.stream()),
                PLAIN[method])
    else:
        N.check(N.lib().mvr_icp_refine_robust(*head, RO.METHODS.index(method), max_dist, epsilon,
                                              RO.KERNELS.index(kernel), 0.0 if k is None else k, max_iters, tol, tol,
                                              *outs, N.ptr(ws), N.stream()), "mvr_icp_refine_robust")
    T4 = np.tile(np.eye(4), (P, 1, 1))
    T4[:, :3] = T.cpu().numpy().reshape(P, 3, 4)
    out = {"T": T4, "fitness": fit.cpu().numpy(), "rmse": rm.cpu().numpy(), "n_corr": nc.cpu().numpy(),
           "iters": it.cpu().numpy(), "status": st.cpu().numpy(), "trace": tr.cpu().numpy()}
    if not plain:
        out["w_sum"] = ws.cpu().numpy()
    return out


def _compare(got, want, rows=None):
    """rows: the pairs compared in full (None: all); the others up to their first evaluation"""
    worst = 0.0
    for k, w in enumerate(want):
        if rows is not None and k not in rows:
            assert not int(got["status"][k]) & 4 and abs(got["trace"][k][0] - w["trace"][0]).max() <= TOL, k
            continue
        for name in ("n_corr", "iters", "status"):
            assert int(got[name][k]) == w[name], (k, name, int(got[name][k]), w[name])
        if w["status"] & 4:      # T0 (possibly not finite) copied bit for bit
            assert got["T"][k][:3].tobytes() == np.ascontiguousarray(w["T"]).tobytes(), k
        dT = 0.0 if w["status"] & 4 else np.abs(got["T"][k][:3] - w["T"]).max()
        df, dr = abs(got["fitness"][k] - w["fitness"]), abs(got["rmse"][k] - w["rmse"])
        dtr = np.abs(got["trace"][k] - w["trace"]).max()
        dw = abs(got["w_sum"][k] - w["w_sum"]) / max(abs(w["w_sum"]), 1e-300)
        print("pair %d: |dT| %.3g, |d fitness| %.3g, |d rmse| %.3g, |d trace| %.3g, rel |d w_sum| %.3g, iters %d, "
              "status %d, n_corr %d, cond %.3g" % (k, dT, df, dr, dtr, dw, w["iters"], w["status"], w["n_corr"],
                                                  max(w["cond"] + [0.0])))
        worst = max(worst, dT, df, dr, dtr, dw)
        assert dT <= TOL and df <= TOL and dr <= TOL and dtr <= TOL and dw <= TOL, k
        np.testing.assert_array_equal(got["T"][k][3], [0.0, 0.0, 0.0, 1.0])
    print("largest difference against the oracle: %.3g" % worst)


# --------------------------------------------------------------------------------------------------- 1. l2, bit for bit
@pytest.mark.parametrize("method", RO.METHODS)
def test_l2_is_bit_identical_to_the_plain_entry(gpu, method):
    fo, T6 = _fo(), _six_starts()
    for iters, tol in ((30, 0.0), (30, 1e-6)):
        plain = _raw(fo, method, None, None, O.SIX, T6, 0.075, iters, tol, plain=True)
        l2 = _raw(fo, method, "l2", None, O.SIX, T6, 0.075, iters, tol)
        for name in NAMES:
            assert not np.any(l2[name] == SENTINEL) and l2[name].tobytes() == plain[name].tobytes(), (name, iters, tol)
        np.testing.assert_array_equal(l2["w_sum"], l2["n_corr"].astype(np.float64))
        assert (l2["n_corr"] > 500).all() and (l2["iters"] > 0).all()         # the runs are no empty ones


# --------------------------------------------------------------------------------------------------- 2. oracle parity
@pytest.mark.parametrize("method", RO.METHODS)
@pytest.mark.parametrize("kernel", RO.KERNELS[1:])
def test_every_kernel_matches_the_oracle(gpu, method, kernel):
    """the six pairs with the tolerances at 1e-6 under a cap of 30 (some pair stops on them, except for Tukey's
    point-to-point loop: test_icp_robust_host.py) and under a cap of 3 (every pair hits it)"""
    fo, T6, k = _fo(), _six_starts(), RO.SCENE_K[kernel]
    pts, nrm = _split(fo, fo.xyz), _split(fo, fo.normals)
    for iters in (30, 3):
        got = _raw(fo, method, kernel, k, O.SIX, T6, 0.075, iters, 1e-6)
        want = RO.icp_robust_batch(method, pts, nrm, O.SIX, T6, 0.075, kernel, k, iters, 1e-6, 1e-6)
        _compare(got, want)
        for j, w in enumerate(want):                                    # -1 in the rows after the last evaluation
            assert (got["trace"][j][w["iters"] + 1:] == -1.0).all() and (got["trace"][j][:w["iters"] + 1] >= 0).all()
        assert all(w["status"] in (0, 2) for w in want)
        if iters == 3:
            assert all(w["status"] == 2 and w["iters"] == 3 for w in want)
    l2 = _raw(fo, method, "l2", None, O.SIX, T6, 0.075, 3, 1e-6)
    assert not np.array_equal(got["T"], l2["T"]) and (got["w_sum"] != l2["w_sum"]).all()    # the kernel: in the solve
    np.testing.assert_array_equal(got["trace"][:, 0], l2["trace"][:, 0])                    # and only the solve


# ----------------------------------------------------------------------------------- 3. small shapes and status bits
@functools.lru_cache(maxsize=None)
def _small():
    """icp_oracle.small_case, icp_plane_oracle.corner_case and small_normals_case with small_normals_pairs as the
    fragments of one index of cell 0.1 (every case's own cell), with normals over 0.1, and their pairs as one batch
    -> (fo, frags, pairs, T0, first row of each case)"""
    from lib.overlap import FragmentOverlap
    frags, pairs, T0, first = [], [], [], []
    for f, p, t in (O.small_case(), PO.corner_case(), (PO.small_normals_case(),) + PO.small_normals_pairs()):
        first.append(len(pairs))
        pairs += (np.asarray(p) + len(frags)).tolist()
        T0 += list(np.asarray(t, np.float64))
        frags += list(f)
    fo = FragmentOverlap(frags, "3DMatch", radius=0.1)
    fo.estimate_normals()
    return fo, frags, np.asarray(pairs), np.asarray(T0), first


@pytest.mark.parametrize("method", RO.METHODS)
def test_small_shapes_and_status_bits_in_one_batch(gpu, method):
    fo, frags, pairs, T0, (ia, ib, ic) = _small()
    pts, nrm = _split(fo, fo.xyz), _split(fo, fo.normals)
    assert [len(frags[s]) for s, _ in pairs[ia:ib]] == [0, 1, 2, 3, 63, 64, 65, 1025, 40]
    assert [len(frags[s]) for s, _ in pairs[ib:ic]] == [0, 1, 5, 6, 63, 64, 65, 1025, 40, 80]
    # two invalid pairs among the others: a NaN in T0 (with a payload), a fragment index B
    T_nan = T0[4].copy()
    T_nan[1, 2] = np.frombuffer(np.uint64(0x7FF8000000ABCDEF).tobytes(), np.float64)[0]
    bad = (3, 12)
    pairs = np.concatenate([pairs[:3], pairs[4:5], pairs[3:11], [[len(frags), 0]], pairs[11:]])
    T0 = np.concatenate([T0[:3], T_nan[None], T0[3:11], T0[5:6], T0[11:]])
    k = 0.03
    want = RO.icp_robust_batch(method, pts, nrm, pairs, T0, 0.1, "tukey", k, 30, 0.0, 0.0)
    got = _raw(fo, method, "tukey", k, pairs, T0, 0.1, 30, 0.0)
    for name in got:
        assert not np.any(got[name] == SENTINEL), name                  # every row of every output is written
    least = RO.MIN_CORR[method]
    full = [j for j, w in enumerate(want) if max(w["cond"] + [0.0]) <= COND_MAX]
    print("status %s\nn_corr %s\ncompared in full: %d of %d" % ([w["status"] for w in want],
                                                                [w["n_corr"] for w in want], len(full), len(want)))
    _compare(got, want, full)
    assert [want[j]["status"] for j in bad] == [4, 4] and all(j in full for j in bad)
    assert {0, 1}.issubset({w["status"] for w in want})
    if method == "point_to_plane":
        assert want[ib + 9 + 2]["status"] == 8                          # the planar target: H has zero rows
    for j in (5, 6, 7, 8, ib + 6, ib + 7, ib + 8, ib + 9):              # the sources of 63, 64, 65 and 1025 points
        assert len(frags[pairs[j][0]]) >= 63 and j in full and want[j]["iters"] == 30 and want[j]["status"] == 0, j
    for j, w in enumerate(want):
        if j in bad:             # invalid: T0 copied bit for bit, everything else 0, no evaluation in the trace
            assert got["T"][j][:3].tobytes() == np.ascontiguousarray(T0[j][:3]).tobytes()
            assert (got["fitness"][j], got["rmse"][j], got["n_corr"][j], got["iters"][j], got["w_sum"][j]) == \
                (0.0, 0.0, 0, 0, 0.0)
            assert (got["trace"][j] == -1.0).all()
        elif w["iters"] == 0:    # too few correspondences, or a refused first solve: T = T0
            assert j in full and (w["n_corr"] < least or w["status"] & 8) and got["iters"][j] == 0
            assert got["T"][j][:3].tobytes() == np.ascontiguousarray(T0[j][:3]).tobytes()
            assert (got["trace"][j][1:] == -1.0).all()
    # the neighbours of the invalid pairs are what they are without them
    ok = [j for j in range(len(pairs)) if j not in bad]
    alone = _raw(fo, method, "tukey", k, pairs[ok], T0[ok], 0.1, 30, 0.0)
    for name in alone:
        assert alone[name].tobytes() == got[name][ok].tobytes(), name
    # once more with a k below every residual of a pair that has correspondences (the 65-point source against the
    # corner): every weight is 0, so the solve is refused, bit 8, T kept bit for bit
    j = ib + 6 + 2
    s, t = pairs[j]
    assert len(frags[s]) == 65 and want[j]["n_corr"] >= 60
    r = np.abs(RO.residuals(method, pts[s], pts[t], nrm[s], nrm[t], T0[j], 0.1))
    tiny = 0.5 * r.min()
    assert tiny > 0
    w0 = RO.icp_robust_batch(method, pts, nrm, pairs[j:j + 1], T0[j:j + 1], 0.1, "tukey", tiny, 30, 0.0, 0.0)
    g0 = _raw(fo, method, "tukey", tiny, pairs[j:j + 1], T0[j:j + 1], 0.1, 30, 0.0)
    _compare(g0, w0)
    assert g0["status"][0] == 8 and g0["iters"][0] == 0 and g0["w_sum"][0] == 0.0
    assert g0["n_corr"][0] == want[j]["n_corr"]
    assert g0["T"][0][:3].tobytes() == np.ascontiguousarray(T0[j][:3]).tobytes() and (g0["trace"][0][1:] == -1.0).all()
    assert g0["trace"][0][0].tobytes() == got["trace"][j][0].tobytes()


# ------------------------------------------------------------------------------------------------- 4. batch invariance
@pytest.mark.parametrize("method", RO.METHODS)
def test_outputs_do_not_depend_on_the_batch(gpu, method):
    fo, T6 = _fo(), _six_starts()
    six = np.asarray(O.SIX)
    ref = _raw(fo, method, "tukey", 0.025, six, T6, 0.075, 30, 0.0)

    def same(rows, where):
        got = _raw(fo, method, "tukey", 0.025, six[rows], T6[rows], 0.075, 30, 0.0)
        for name in ref:
            assert got[name].tobytes() == np.ascontiguousarray(ref[name][rows]).tobytes(), (where, name)

    for j in range(6):                                                  # each pair alone
        same([j], "alone %d" % j)
    same(np.random.default_rng(1).permutation(6), "shuffled")
    same(np.array([0, 1, 2, 0, 1, 0, 5, 2, 2, 0, 0]), "repeated")       # fragment 0 the source of several pairs


# ------------------------------------------------------------------------------------------- 5. translation invariance
@pytest.mark.parametrize("method", RO.METHODS)
def test_translation_invariance(gpu, method):
    """Every fragment moved by icp_plane_oracle.SHIFT, the starts conjugated: T conjugated back agrees with the
    unshifted run within the bound of the method's own translation test: 1e-7 for point-to-plane (point-to-point has
    none: the same, its sums have per-pair origins too), 1e-9 for generalized."""
    from lib.overlap import FragmentOverlap
    bound = TOL if method == "generalized" else 1e-7
    pts = _split(_fo(), _fo().xyz)
    T6 = _six_starts()
    out = []
    for shift in (np.zeros(3), PO.SHIFT):
        fo = FragmentOverlap([p + shift for p in pts], "3DMatch", radius=0.075)
        fo.estimate_normals()
        got = _raw(fo, method, "tukey", 0.025, O.SIX, PO.conjugate_starts(T6, shift), 0.075, 30, 0.0)
        assert (got["status"] == 0).all() and (got["iters"] == 30).all()
        out.append((PO.conjugate_starts(got["T"], -shift), got["n_corr"], got["w_sum"]))
    diff = np.abs(out[0][0] - out[1][0]).max()
    print("shifted by %s and conjugated back against unshifted: %.3g; w_sum relative %.3g"
          % (PO.SHIFT.tolist(), diff, np.abs(out[0][2] / out[1][2] - 1.0).max()))
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert diff <= bound


# -------------------------------------------------------------------------------------------------------- 6. robustness
@pytest.mark.parametrize("method", RO.METHODS)
def test_tukey_at_least_halves_the_error_on_the_contaminated_case(gpu, method):
    """icp_robust_oracle.contaminated_case: 30 % of the source displaced by 6 cm inside max_dist 0.1.  The oracle
    meets the factor for the generalized loop too (test_icp_robust_host.py has the figures), so it is asserted for
    all three methods."""
    from lib.overlap import FragmentOverlap
    src, tgt, Tt, T0 = RO.contaminated_case()
    fo = FragmentOverlap([src, tgt], "3DMatch", radius=PO.CORNER_RADIUS)
    fo.estimate_normals()
    pts, nrm = _split(fo, fo.xyz), _split(fo, fo.normals)
    err = {}
    for kernel, k in (("l2", None), ("tukey", RO.CONTAMINATED_K)):
        got = _raw(fo, method, kernel, k, [[0, 1]], T0[None], RO.CONTAMINATED_MAX_DIST, RO.CONTAMINATED_ITERS, 0.0)
        want = RO.icp_robust_batch(method, pts, nrm, [[0, 1]], T0[None], RO.CONTAMINATED_MAX_DIST, kernel, k,
                                   RO.CONTAMINATED_ITERS, 0.0, 0.0)
        _compare(got, want)
        err[kernel] = RO.motion_error(got["T"][0], Tt, tgt)
    print("%s: largest displacement of a target point, l2 %.3g mm, tukey %.3g mm"
          % (method, 1e3 * err["l2"], 1e3 * err["tukey"]))
    assert err["tukey"] <= 0.5 * err["l2"]


# ---------------------------------------------------------------------------------------------------- 7. Python surface
def test_python_surface_dtypes_and_devices(gpu):
    import torch
    from lib.icp import gicp_pair, gicp_refine, icp_pair, icp_refine
    fo, T6 = _fo(), _six_starts()
    calls = {"point_to_point": lambda *a, **kw: icp_refine(fo, *a, **kw),
             "point_to_plane": lambda *a, **kw: icp_refine(fo, *a, method="point_to_plane", **kw),
             "generalized": lambda *a, **kw: gicp_refine(fo, *a, **kw)}
    for method, call in calls.items():
        ref = _raw(fo, method, "tukey", 0.025, O.SIX, T6, 0.075, 30, 1e-6)
        # fp64 torch on the device in -> torch on the device out, the same bits as the raw call
        dev = call(torch.tensor(O.SIX, device=gpu), torch.from_numpy(T6).to(gpu), 0.075, return_trace=True,
                   kernel="tukey", kernel_k=0.025, return_weight_sum=True)
        assert all(torch.is_tensor(v) and v.device.type == "cuda" for v in dev.values()) and set(dev) == set(ref)
        assert dev["T"].shape == (6, 4, 4) and dev["trace"].shape == (6, 31, 2) and dev["w_sum"].shape == (6,)
        assert dev["w_sum"].dtype == torch.float64 and dev["n_corr"].dtype == torch.int32
        for name in ref:
            assert dev[name].cpu().numpy().tobytes() == ref[name].tobytes(), (method, name)
        # [P,3,4] and fp32 inputs (torch on the host -> torch on the host, numpy -> numpy): the fp32 start, in fp64
        T32 = T6[:, :3].astype(np.float32)
        want = call(O.SIX, T32.astype(np.float64), 0.075, kernel="huber", kernel_k=0.025)
        assert "w_sum" not in want and "trace" not in want
        for Tin in (torch.from_numpy(T32), T32):
            out = call(O.SIX, Tin, 0.075, kernel="huber", kernel_k=0.025)
            assert all((torch.is_tensor(v) and v.device.type == "cpu") if torch.is_tensor(Tin) else
                       isinstance(v, np.ndarray) for v in out.values())
            for name in want:
                assert np.asarray(out[name]).tobytes() == want[name].tobytes(), (method, name)
        # kernel=None is the plain entry, the same bytes as before; 'l2' is the new entry with the same bytes
        plain = _raw(fo, method, None, None, O.SIX, T6, 0.075, 30, 1e-6, plain=True)
        none = call(O.SIX, T6, 0.075, return_trace=True)
        l2 = call(O.SIX, T6, 0.075, return_trace=True, kernel="l2", return_weight_sum=True)
        assert "w_sum" not in none
        for name in NAMES:
            assert none[name].tobytes() == plain[name].tobytes() == l2[name].tobytes(), (method, name)
        np.testing.assert_array_equal(l2["w_sum"], l2["n_corr"])
        assert not np.array_equal(none["T"], ref["T"])
    # the one-pair shapes pass the kernel on
    src, tgt, T_one, max_dist, iters = O.pair_case()
    for pair, kw in ((icp_pair, {}), (icp_pair, {"method": "point_to_plane"}), (gicp_pair, {})):
        a = pair(src, tgt, T_one, max_dist=max_dist, max_iters=iters, **kw)
        b = pair(src, tgt, T_one, max_dist=max_dist, max_iters=iters, kernel="l2", return_weight_sum=True, **kw)
        c = pair(src, tgt, T_one, max_dist=max_dist, max_iters=iters, kernel="cauchy", kernel_k=0.01, **kw)
        assert a["T"].tobytes() == b["T"].tobytes() and b["w_sum"] == b["n_corr"] and b["w_sum"].shape == ()
        assert c["T"].shape == (4, 4) and not np.array_equal(a["T"], c["T"]) and np.isfinite(c["T"]).all()


def test_register_scene_passes_the_kernel_to_the_icp_stage(gpu):
    """three fragments of the scene with the pairwise starts given: the pairs' T are those of a direct icp_refine call
    with k = voxel_size on the chain's own index, and None leaves the chain as it is"""
    from lib.icp import gicp_refine, icp_refine
    from lib.multiview import register_scene
    raw = O.scene4()[0][:3]
    pairs = [(0, 1), (0, 2), (1, 2)]
    init = np.asarray([_six_starts()[O.SIX.index(p)] for p in pairs])
    for method in RO.METHODS:
        res = register_scene(raw, 0.025, method=method, init=init, icp_kernel="tukey")
        rec, fo = res["pairs"], res["fo"]
        kept = rec["kept"]
        assert np.isfinite(res["poses"]).all() and kept.any()
        kw = dict(max_iters=30, kernel="tukey", kernel_k=0.025)
        direct = gicp_refine(fo, pairs, init, **kw) if method == "generalized" else \
            icp_refine(fo, pairs, init, method=method, **kw)
        assert rec["T"][kept].tobytes() == np.asarray(direct["T"])[kept].tobytes(), method
        assert not np.array_equal(rec["T"][kept], init[kept])
    assert rec["T"].tobytes() == register_scene(raw, 0.025, method=method, init=init, icp_kernel="tukey",
                                                icp_kernel_k=0.025)["pairs"]["T"].tobytes()
    plain = register_scene(raw, 0.025, init=init)
    none = register_scene(raw, 0.025, init=init, icp_kernel=None, icp_kernel_k=None)
    assert plain["pairs"]["T"].tobytes() == none["pairs"]["T"].tobytes() and plain["poses"].tobytes() == \
        none["poses"].tobytes()
    assert not np.array_equal(plain["pairs"]["T"], res["pairs"]["T"])
