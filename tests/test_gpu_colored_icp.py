"""GPU coloured ICP (csrc/icp_colored.hip mvr_icp_refine_colored, lib.icp.colored_icp_refine / colored_icp_pair), its
colour gradients (csrc/color_grad.hip mvr_color_gradient, FragmentOverlap.compute_color_gradients) and the colours of
FragmentOverlap (csrc/overlap.hip mvr_voxel_centroids_colored) against the numpy / sklearn oracle
(tests/colored_icp_oracle.py): voxel colours, gradients on the scene, on a linear field and on small and awkward
shapes, fixed iteration counts with the full trace, convergence, the status bits, lambda = 1 against point-to-plane, the
textured plane that geometry alone cannot register, the robust kernels, batch and translation invariance, the Python
surface and register_scene(method='colored').

Tolerance: the project's fp64 bound 1e-9 on gradients, T, fitness, rmse, the trace and (relative) w_sum; intensities
bit for bit; n_nbr, n_corr, iters and status exactly.  The comparisons feed the oracle the GPU's own normals (and, for
the loop, gradients), so the eigen-solver's sign and rounding stay out of them.  test_colored_icp_host.py checks that
no case used here has a neighbour, a correspondence, a stopping test or a pivot test within rounding of a tie."""
import functools

import numpy as np
import pytest

import colored_icp_oracle as CO
import icp_oracle as O
import icp_plane_oracle as PO
import icp_robust_oracle as RO

pytestmark = pytest.mark.gpu
TOL = 1e-9
SENTINEL = -77.0
NAMES = ("T", "fitness", "rmse", "n_corr", "iters", "status", "trace")


@functools.lru_cache(maxsize=None)
def _fo():
    """the scene's coloured centroids on an index of cell 0.075, with normals and gradients over that radius"""
    from lib.overlap import FragmentOverlap
    fo = FragmentOverlap(O.scene4()[0], "FCGF", 0.025, colors=CO.scene4_raw_colors())
    fo.estimate_normals()
    fo.compute_color_gradients()
    return fo


def _split(fo, x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    return [x[fo.off[b]:fo.off[b + 1]] for b in range(fo.B)]


def _inputs(fo):
    """what the oracle's loop takes, from the GPU object: points, normals, intensities, gradients per fragment"""
    return _split(fo, fo.xyz), _split(fo, fo.normals), _split(fo, fo.intensity), _split(fo, fo.color_grad)


@functools.lru_cache(maxsize=None)
def _six_starts():
    return O.scene4_starts(O.SIX, O.scene4_centroids())


@functools.lru_cache(maxsize=None)
def _six(max_dist, max_iters, tol, kernel=None, lam=CO.LAMBDA):
    """(GPU result with trace and w_sum, oracle results on the GPU's inputs) of the six pairs"""
    from lib.icp import colored_icp_refine
    fo = _fo()
    k = None if kernel in (None, "l2") else CO.ROBUST_K
    got = colored_icp_refine(fo, O.SIX, _six_starts(), max_dist, max_iters, tol, tol, lambda_geometric=lam,
                             kernel=kernel, kernel_k=k, return_trace=True, return_weight_sum=True)
    want = CO.colored_icp_batch(*_inputs(fo), O.SIX, _six_starts(), max_dist, lam, kernel or "l2", k, max_iters, tol,
                                tol)
    return got, want


def _compare(got, want, trace=True):
    for k, w in enumerate(want):
        for name in ("n_corr", "iters", "status"):
            assert int(got[name][k]) == w[name], (k, name, int(got[name][k]), w[name])
        if w["status"] & 4:      # T0 (possibly not finite) copied bit for bit
            assert got["T"][k][:3].tobytes() == np.ascontiguousarray(w["T"]).tobytes(), k
        dT = 0.0 if w["status"] & 4 else np.abs(got["T"][k][:3] - w["T"]).max()
        df, dr = abs(got["fitness"][k] - w["fitness"]), abs(got["rmse"][k] - w["rmse"])
        dtr = np.abs(got["trace"][k] - w["trace"]).max() if trace else 0.0
        dw = abs(got["w_sum"][k] - w["w_sum"]) / max(abs(w["w_sum"]), 1.0) if "w_sum" in got else 0.0
        print("pair %d: |dT| %.3g, |d fitness| %.3g, |d rmse| %.3g, |d trace| %.3g, rel |d w_sum| %.3g, iters %d, "
              "status %d, n_corr %d, smallest pivot ratio %.3g"
              % (k, dT, df, dr, dtr, dw, w["iters"], w["status"], w["n_corr"], min(w["pivots"] + [np.inf])))
        assert dT <= TOL and df <= TOL and dr <= TOL and dtr <= TOL and dw <= TOL, k
        np.testing.assert_array_equal(got["T"][k][3], [0.0, 0.0, 0.0, 1.0])


# ------------------------------------------------------------------------------------------------------ voxel colours
def test_voxel_colours_and_select(gpu):
    import torch
    from lib.overlap import FragmentOverlap
    fo = _fo()
    plain = FragmentOverlap(O.scene4()[0], "FCGF", 0.025)
    assert plain.colors is None and fo.colors.dtype == torch.float64 and tuple(fo.colors.shape) == (fo.M, 3)
    assert fo.xyz.cpu().numpy().tobytes() == plain.xyz.cpu().numpy().tobytes()      # the same passes: bit-identical
    assert fo.off.tobytes() == plain.off.tobytes()
    cent, col = CO.scene4_colored_centroids()
    assert [len(c) for c in cent] == np.diff(fo.off).tolist()
    d_xyz = np.abs(np.concatenate(cent) - fo.xyz.cpu().numpy()).max()               # the oracle's rows are the GPU's
    d_col = np.abs(np.concatenate(col) - fo.colors.cpu().numpy()).max()
    print("voxel colours: %d voxels, |d xyz| %.3g, |d colour| %.3g against the per-voxel mean in input order"
          % (fo.M, d_xyz, d_col))
    assert d_xyz <= 1e-12 and d_col <= 1e-12
    # select: a row gather of the colours, the gradients reset as the normals are
    keep = np.random.default_rng(0).random(fo.M) < 0.6
    sel = fo.select(keep)
    assert sel.colors.cpu().numpy().tobytes() == fo.colors.cpu().numpy()[keep].tobytes() and sel.colors.is_contiguous()
    assert sel.intensity is None and sel.color_grad is None and sel.normals is None
    assert plain.select(keep).colors is None
    # raw points: the caller's rows, uint8 divided by 255
    pts = [f[:50] for f in O.scene4()[0][:2]]
    u8 = [np.random.default_rng(b).integers(0, 256, (50, 3)).astype(np.uint8) for b in range(2)]
    raw = FragmentOverlap(pts, "3DMatch", colors=u8)
    assert raw.colors.cpu().numpy().tobytes() == (np.concatenate(u8).astype(np.float64) / 255.0).tobytes()
    as_float = FragmentOverlap(pts, "3DMatch", colors=[c / 255.0 for c in u8])
    assert as_float.colors.cpu().numpy().tobytes() == raw.colors.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="colors"):
        FragmentOverlap(pts, "3DMatch", colors=u8[:1])
    with pytest.raises(ValueError, match="colors"):
        FragmentOverlap(pts, "3DMatch", colors=[u8[0], u8[1][:40]])


# ---------------------------------------------------------------------------------------------------------- gradients
def _raw_gradients(fo, radius, normals=None):
    """mvr_color_gradient on sentinel-filled output buffers -> (intensity [M], grad [M,3], n_nbr [M]) numpy"""
    import torch
    from lib import _native as N
    nrm = fo.normals if normals is None else normals
    I = torch.full((fo.M,), SENTINEL, dtype=torch.float64, device=fo.device)
    g = torch.full((fo.M, 3), SENTINEL, dtype=torch.float64, device=fo.device)
    cnt = torch.full((fo.M,), int(SENTINEL), dtype=torch.int32, device=fo.device)
    N.check(N.lib().mvr_color_gradient(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(nrm), N.ptr(fo.colors),
                                       N.ptr(fo.off_dev), fo.B, fo.M, fo.r, radius, N.ptr(I), N.ptr(g), N.ptr(cnt),
                                       N.stream()), "mvr_color_gradient")
    return I.cpu().numpy(), g.cpu().numpy(), cnt.cpu().numpy()


def _compare_gradients(what, fo, got, radius, max_left_out):
    """intensity bit for bit, n_nbr exactly, gradients within TOL except where the oracle's pivot ratio lies within
    100 x of the floor -> the oracle's per-fragment dicts"""
    I, g, cnt = got
    want = CO.color_gradients_batch(_split(fo, fo.xyz), _split(fo, fo.normals), _split(fo, fo.colors), radius)
    w_I, w_g = np.concatenate([w["intensity"] for w in want]), np.concatenate([w["grad"] for w in want])
    w_c, piv = np.concatenate([w["n_nbr"] for w in want]), np.concatenate([w["pivot"] for w in want])
    nan = np.isnan(w_I)                                                 # bit for bit, a NaN where the oracle has one
    np.testing.assert_array_equal(np.isnan(I), nan)
    assert I[~nan].tobytes() == w_I[~nan].tobytes()
    np.testing.assert_array_equal(cnt, w_c)
    assert not np.any(g == SENTINEL) and np.isfinite(g).all()
    out = CO.near_floor(piv)
    diff = np.abs(g - w_g).max(1) if len(g) else np.zeros(0)
    solved = piv[np.isfinite(piv) & (piv > CO.PIVOT_FLOOR)]
    print("%s: %d points, neighbours %d..%d, smallest pivot ratio of a solve %.3g, %d left out near the floor, largest "
          "gradient %.3g, largest difference %.3g" % (what, len(g), w_c.min(), w_c.max(), solved.min() if len(solved)
                                                      else np.inf, int(out.sum()), np.abs(w_g).max(),
                                                      diff[~out].max() if (~out).any() else 0.0))
    assert out.mean() <= max_left_out
    assert (diff[~out] <= TOL).all()
    np.testing.assert_array_equal(g[w_c < 4], 0.0)
    return want


@pytest.mark.parametrize("radius", [0.075, 0.05])
def test_scene_gradients_match_oracle(gpu, radius):
    fo = _fo()
    assert fo.r == 3 * 0.025 and all(2270 <= n <= 2687 for n in np.diff(fo.off))
    got = _raw_gradients(fo, radius)
    want = _compare_gradients("scene, radius %g" % radius, fo, got, radius, 0.0)
    assert np.concatenate([w["n_nbr"] for w in want]).min() >= 4 and np.abs(got[1]).max() > 1.0
    # the normals' sign does not matter: the same bits
    flipped = _raw_gradients(fo, radius, normals=(-fo.normals).contiguous())
    for a, b in zip(got, flipped):
        assert a.tobytes() == b.tobytes()
    if radius == 0.075:      # FragmentOverlap.compute_color_gradients: the same call, stored on the object
        assert fo.intensity.cpu().numpy().tobytes() == got[0].tobytes()
        assert fo.color_grad.cpu().numpy().tobytes() == got[1].tobytes()
        assert fo.color_n_nbr.cpu().numpy().tobytes() == got[2].tobytes()


@pytest.mark.parametrize("tilted", [False, True])
def test_linear_field_gives_its_own_gradient(gpu, tilted):
    """I = 0.3 + a . x exactly on 4000 points of a plane: every gradient is a - (a . n) n, to 1e-12 on the plane
    z = 0.3 (the oracle: 4.2e-15).  On the tilted plane the heavy row (n_nbr - 1) n . d = 0 enters every entry of A
    and the stated Cholesky loses the digits of A's condition (pivot ratio 2e-5; the oracle: 1.9e-12): there the
    bound is the project's 1e-9."""
    import torch
    from lib.overlap import FragmentOverlap
    pts, n, colors, a = CO.linear_field_case(tilted)
    fo = FragmentOverlap([pts], "3DMatch", radius=0.075, colors=[colors])
    fo.normals = torch.as_tensor(np.tile(n, (len(pts), 1))).to(fo.device).contiguous()
    out = fo.compute_color_gradients()
    assert int(out["n_nbr"].min()) >= 4
    diff = np.abs(out["grad"].cpu().numpy() - (a - (a @ n) * n)).max()
    print("linear field%s: neighbours %d..%d, largest |gradient - (a - (a . n) n)| %.3g"
          % (", tilted" if tilted else "", int(out["n_nbr"].min()), int(out["n_nbr"].max()), diff))
    assert diff <= (TOL if tilted else 1e-12)


def test_gradients_on_small_shapes_in_one_batch(gpu):
    from lib.overlap import FragmentOverlap
    frags, colors = CO.small_colored_case()
    fo = FragmentOverlap(frags, "3DMatch", radius=PO.SMALL_R_INDEX, colors=colors)
    assert tuple(np.diff(fo.off)) == PO.SMALL_SIZES + (4, 64)
    fo.estimate_normals()
    nb, row = CO.SMALL_NAN
    for radius in (0.06, PO.SMALL_R_INDEX):                                     # radius < r_index, radius == r_index
        got = _raw_gradients(fo, radius)                                        # every row written over the sentinel
        want = _compare_gradients("small shapes, radius %g" % radius, fo, got, radius, 0.05)
        g, c = _split(fo, got[1]), _split(fo, got[2])
        for b in (1, 2, 3):                                                     # below 4 neighbours: 0
            assert (c[b] < 4).all() and not g[b].any()
        assert (c[CO.SMALL_FOUR] == 4).all()
        assert (c[CO.SMALL_LINE] >= 4).all() and not g[CO.SMALL_LINE].any()      # collinear: the failed pivot
        assert (want[CO.SMALL_LINE]["pivot"] < CO.PIVOT_FLOOR / 10.0).all()
        # the NaN colour: gradient 0 for the points whose ball holds it, and only for those
        assert np.isnan(_split(fo, got[0])[nb][row]) and np.isfinite(np.delete(got[0], fo.off[nb] + row)).all()
        holds = want[nb]["nan"]
        assert holds[row] and 1 < holds.sum() < len(holds) and not g[nb][holds].any()
        assert g[nb][~holds & (c[nb] >= 4)].any(1).mean() > 0.9
    # a fragment's outputs do not depend on the fragments around it
    whole = _raw_gradients(fo, PO.SMALL_R_INDEX)
    for b in (nb, CO.SMALL_FOUR):
        alone = FragmentOverlap([frags[b]], "3DMatch", radius=PO.SMALL_R_INDEX, colors=[colors[b]])
        alone.normals = fo.normals[fo.off[b]:fo.off[b + 1]].clone()
        one = _raw_gradients(alone, PO.SMALL_R_INDEX)
        for a, w in zip(one, whole):
            assert a.tobytes() == _split(fo, w)[b].tobytes()


# ------------------------------------------------------------------------------------------------- fixed iterations
@pytest.mark.parametrize("max_dist", [0.075, 0.03])
def test_thirty_iterations_match_oracle_with_trace(gpu, max_dist):
    """max_dist 0.03 on the index of cell 0.075: the search ball is smaller than the cell"""
    got, want = _six(max_dist, 30, 0.0)
    assert all(w["iters"] == 30 and w["status"] == 0 for w in want)
    _compare(got, want)
    assert (got["trace"] >= 0).all()


def test_convergence_and_iteration_cap(gpu):
    got, want = _six(0.075, 30, 1e-6)
    assert all(w["status"] == 0 and 0 < w["iters"] < 30 for w in want)
    _compare(got, want)
    for k, w in enumerate(want):                                        # -1 in the rows after the last evaluation
        assert (got["trace"][k][w["iters"] + 1:] == -1.0).all() and (got["trace"][k][:w["iters"] + 1] >= 0).all()
    got3, want3 = _six(0.075, 3, 1e-6)
    assert all(w["status"] == 2 and w["iters"] == 3 for w in want3)
    _compare(got3, want3)


# -------------------------------------------------------------------------------------------------------- status bits
def _raw_call(fo, pairs, T0, max_dist, max_iters, tol, lam=CO.LAMBDA, kernel=0, k=0.0):
    """mvr_icp_refine_colored on sentinel-filled output buffers -> numpy outputs"""
    import torch
    from lib import _native as N
    d = fo.device
    P = len(pairs)
    gp = torch.as_tensor(np.asarray(pairs, np.int64)).to(d)
    gT = torch.as_tensor(np.ascontiguousarray(np.asarray(T0, np.float64)[:, :3])).to(d)
    T = torch.full((P, 12), SENTINEL, dtype=torch.float64, device=d)
    fit, rm, ws = (torch.full((P,), SENTINEL, dtype=torch.float64, device=d) for _ in range(3))
    nc, it, st = (torch.full((P,), int(SENTINEL), dtype=torch.int32, device=d) for _ in range(3))
    tr = torch.full((P, max_iters + 1, 2), SENTINEL, dtype=torch.float64, device=d)
    N.check(N.lib().mvr_icp_refine_colored(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.normals),
                                           N.ptr(fo.intensity), N.ptr(fo.color_grad), N.ptr(fo.off_dev), fo.B, fo.M,
                                           fo.r, N.ptr(gp), N.ptr(gT), P, max_dist, lam, kernel, k, max_iters, tol,
                                           tol, N.ptr(T), N.ptr(fit), N.ptr(rm), N.ptr(nc), N.ptr(it), N.ptr(st),
                                           N.ptr(tr), N.ptr(ws), N.stream()), "mvr_icp_refine_colored")
    T4 = np.tile(np.eye(4), (P, 1, 1))
    T4[:, :3] = T.cpu().numpy().reshape(P, 3, 4)
    return {"T": T4, "fitness": fit.cpu().numpy(), "rmse": rm.cpu().numpy(), "n_corr": nc.cpu().numpy(),
            "iters": it.cpu().numpy(), "status": st.cpu().numpy(), "trace": tr.cpu().numpy(),
            "w_sum": ws.cpu().numpy()}


def test_small_shapes_and_status_bits_in_one_batch(gpu):
    from lib.overlap import FragmentOverlap
    frags, pairs, T0 = PO.corner_case()
    fo = FragmentOverlap(frags, "3DMatch", radius=PO.CORNER_RADIUS, colors=CO.corner_colors(frags))
    fo.estimate_normals()
    fo.compute_color_gradients()
    assert not _split(fo, fo.color_grad)[1].any()                       # the constant-colour plane: gradients exactly 0
    # two invalid pairs among the others: a NaN in T0 (with a payload), a fragment index B
    T_nan = T0[4].copy()
    T_nan[1, 2] = np.frombuffer(np.uint64(0x7FF8000000ABCDEF).tobytes(), np.float64)[0]
    pairs = np.concatenate([pairs[:3], [[6, 0]], pairs[3:6], [[len(frags), 0]], pairs[6:]])
    T0 = np.concatenate([T0[:3], T_nan[None], T0[3:6], T0[5:6], T0[6:]])
    want = CO.colored_icp_batch(*_inputs(fo), pairs, T0, PO.CORNER_RADIUS, max_iters=30, tol_fitness=0.0, tol_rmse=0.0)
    got = _raw_call(fo, pairs, T0, PO.CORNER_RADIUS, 30, 0.0)
    status = [w["status"] for w in want]
    print("statuses %s, n_corr %s, iters %s" % (status, [w["n_corr"] for w in want], [w["iters"] for w in want]))
    assert {0, 1, 4, 8} <= set(status) and status[3] == status[7] == 4 and status[11] == 8
    for name in got:
        assert not np.any(got[name] == SENTINEL), name                  # every row of every output is written
    _compare(got, want)
    for k in (3, 7):             # invalid: T0 copied bit for bit, everything else 0, no evaluation in the trace
        assert got["T"][k][:3].tobytes() == np.ascontiguousarray(T0[k][:3]).tobytes()
        assert (got["fitness"][k], got["rmse"][k], got["n_corr"][k], got["iters"][k], got["w_sum"][k]) == \
            (0.0, 0.0, 0, 0, 0.0)
        assert (got["trace"][k] == -1.0).all()
    for k in [j for j, s in enumerate(status) if s in (1, 8)]:          # no solve went through: T = T0
        assert got["T"][k][:3].tobytes() == np.ascontiguousarray(T0[k][:3]).tobytes() and got["iters"][k] == 0
    np.testing.assert_array_equal(got["w_sum"], got["n_corr"].astype(np.float64))          # unit weights: the count
    # the neighbours of the invalid pairs are what they are without them
    ok = [k for k in range(len(pairs)) if k not in (3, 7)]
    alone = _raw_call(fo, pairs[ok], T0[ok], PO.CORNER_RADIUS, 30, 0.0)
    for name in alone:
        assert alone[name].tobytes() == got[name][ok].tobytes(), name


# ----------------------------------------------------------------------------------------------------------- lambda 1
def test_lambda_one_is_point_to_plane(gpu):
    from lib.icp import colored_icp_refine, icp_refine
    fo, T6 = _fo(), _six_starts()
    kw = dict(max_dist=0.075, max_iters=30, tol_fitness=0.0, tol_rmse=0.0, return_trace=True)
    col = colored_icp_refine(fo, O.SIX, T6, lambda_geometric=1.0, **kw)
    p2l = icp_refine(fo, O.SIX, T6, method="point_to_plane", **kw)
    same = all(col[name].tobytes() == p2l[name].tobytes() for name in NAMES)
    print("lambda = 1 against point-to-plane: largest |dT| %.3g, |d trace| %.3g; the bits agree: %s"
          % (np.abs(col["T"] - p2l["T"]).max(), np.abs(col["trace"] - p2l["trace"]).max(), same))
    for name in ("n_corr", "iters", "status"):
        np.testing.assert_array_equal(col[name], p2l[name])
    for name in ("T", "fitness", "rmse", "trace"):
        assert np.abs(col[name] - p2l[name]).max() <= TOL, name


# ------------------------------------------------------------------------------------------------- the textured plane
def test_textured_plane_needs_the_colours(gpu):
    """The case colour exists for.  The oracle's error against the true motion is 4.1e-5 (from a start 0.060 away;
    a second seed: 6.3e-5); point-to-plane stops at its first solve with status 8 and point-to-point stays 0.062 away.
    The GPU must agree with the oracle within 1e-9, lie within 10 x the oracle's error of the truth (the margin covers
    a differently drawn sample), and point-to-point must stay at least 100 x the oracle's error away."""
    from lib.icp import colored_icp_pair, icp_pair
    from lib.overlap import FragmentOverlap
    src, sc, tgt, tc, Tt = CO.textured_plane_case()
    kw = dict(max_dist=PO.NORMAL_RADIUS, max_iters=CO.PLANE_ITERS, tol_fitness=0.0, tol_rmse=0.0)
    got = colored_icp_pair(src, sc, tgt, tc, np.eye(4), return_trace=True, return_weight_sum=True, **kw)
    fo = FragmentOverlap([src, tgt], "3DMatch", radius=CO.PLANE_RADIUS, colors=[sc, tc])
    fo.estimate_normals()
    fo.compute_color_gradients()
    pts, nrm, I, g = _inputs(fo)
    want = CO.colored_icp(pts[0], pts[1], nrm[1], I[0], I[1], g[1], np.eye(4), CO.PLANE_RADIUS,
                          max_iters=CO.PLANE_ITERS, tol_fitness=0.0, tol_rmse=0.0)
    _compare({k: np.asarray(v)[None] for k, v in got.items()}, [want])
    e_gpu, e_want = CO.motion_error(got["T"], Tt, src), CO.motion_error(want["T"], Tt, src)
    p2l = icp_pair(src, tgt, np.eye(4), method="point_to_plane", **kw)
    p2p = icp_pair(src, tgt, np.eye(4), **kw)
    e_p2p = CO.motion_error(p2p["T"], Tt, src)
    print("textured plane: start %.3g away; coloured %.3g (oracle %.3g, status %d, %d iterations); point-to-plane "
          "status %d after %d iterations; point-to-point %.3g"
          % (CO.motion_error(np.eye(4), Tt, src), e_gpu, e_want, want["status"], want["iters"], int(p2l["status"]),
             int(p2l["iters"]), e_p2p))
    assert want["status"] == 0 and want["iters"] == CO.PLANE_ITERS and e_want < 1e-3
    assert e_gpu <= 10.0 * e_want
    assert e_p2p >= 100.0 * e_want


# ------------------------------------------------------------------------------------------------------ robust kernels
@pytest.mark.parametrize("kernel", RO.KERNELS[1:])
def test_every_kernel_matches_the_oracle(gpu, kernel):
    got, want = _six(0.075, 3, 0.0, kernel)
    assert all(w["iters"] == 3 and w["status"] == 0 for w in want)
    _compare(got, want)
    plain, _ = _six(0.075, 3, 0.0)
    assert not np.array_equal(got["T"], plain["T"])
    assert (got["w_sum"] > 0).all() and not np.array_equal(got["w_sum"], plain["w_sum"])


def test_l2_is_the_plain_launch(gpu):
    plain, _ = _six(0.075, 30, 0.0)
    l2, _ = _six(0.075, 30, 0.0, "l2")
    for name in plain:
        assert plain[name].tobytes() == l2[name].tobytes(), name
    n = plain["n_corr"].astype(np.float64)
    assert (np.abs(plain["w_sum"] - n) <= 1e-9 * n).all() and (n > 500).all()


# --------------------------------------------------------------------------------------------------- batch invariance
def test_outputs_do_not_depend_on_the_batch(gpu):
    from lib.icp import colored_icp_refine
    fo = _fo()
    T6 = _six_starts()
    ref, _ = _six(0.075, 30, 0.0)
    kw = dict(max_dist=0.075, max_iters=30, tol_fitness=0.0, tol_rmse=0.0, return_trace=True, return_weight_sum=True)

    def same(got, rows, where):
        for name in ref:
            assert np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(ref[name][rows]).tobytes(), \
                (where, name)

    for k in range(6):                                                  # each pair alone
        same(colored_icp_refine(fo, [O.SIX[k]], T6[k:k + 1], **kw), [k], "alone %d" % k)
    perm = np.random.default_rng(1).permutation(6)                      # shuffled
    same(colored_icp_refine(fo, np.asarray(O.SIX)[perm], T6[perm], **kw), perm, "shuffled")
    rows = np.array([0, 1, 2, 0, 1, 0, 5, 2, 2, 0, 0])                  # fragment 0 the source of several pairs
    same(colored_icp_refine(fo, np.asarray(O.SIX)[rows], T6[rows], **kw), rows, "repeated")


def test_translation_invariance(gpu):
    """Every fragment moved by (100, -200, 50), the colours kept, the starts conjugated: T conjugated back agrees with
    the unshifted run within 1e-7, as in the plane test (a shift of 2e2 costs about 2e2 eps per coordinate and the
    loop is contractive).  test_colored_icp_host.py checks the oracle's own difference on the CPU first."""
    from lib.overlap import FragmentOverlap
    from lib.icp import colored_icp_refine
    base = _fo()
    pts, cols = _split(base, base.xyz), _split(base, base.colors)
    T6 = _six_starts()
    kw = dict(max_dist=0.075, max_iters=30, tol_fitness=0.0, tol_rmse=0.0)
    out = []
    for shift in (np.zeros(3), PO.SHIFT):
        fo = FragmentOverlap([p + shift for p in pts], "3DMatch", radius=0.075, colors=cols)
        fo.estimate_normals()
        fo.compute_color_gradients()
        got = colored_icp_refine(fo, O.SIX, PO.conjugate_starts(T6, shift), **kw)
        assert (got["status"] == 0).all() and (got["iters"] == 30).all()
        out.append((PO.conjugate_starts(got["T"], -shift), got["n_corr"]))
    diff = np.abs(out[0][0] - out[1][0]).max()
    print("shifted by %s and conjugated back against unshifted: %.3g" % (PO.SHIFT.tolist(), diff))
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert diff <= 1e-7
    ref, _ = _six(0.075, 30, 0.0)                                       # the raw-point index holds the same points
    assert np.abs(out[0][0] - ref["T"]).max() <= TOL


# ----------------------------------------------------------------------------------------------------- Python surface
def test_python_surface_dtypes_and_devices(gpu):
    import torch
    from lib.icp import METHODS, colored_icp_pair, colored_icp_refine
    from lib.overlap import FragmentOverlap
    assert METHODS == ("point_to_point", "point_to_plane")              # a function of its own, as gicp_refine
    fo = _fo()
    T6 = _six_starts()
    ref, _ = _six(0.075, 30, 1e-6)
    assert fo.intensity.dtype == torch.float64 and fo.intensity.device.type == "cuda" and fo.intensity.shape == (fo.M,)
    assert fo.color_grad.dtype == torch.float64 and fo.color_grad.shape == (fo.M, 3)
    assert fo.color_n_nbr.dtype == torch.int32 and fo.color_n_nbr.shape == (fo.M,)
    # fp64 torch on the device in -> torch on the device out, the same bits
    dev_out = colored_icp_refine(fo, torch.tensor(O.SIX, device=gpu), torch.from_numpy(T6).to(gpu), 0.075,
                                 return_trace=True, return_weight_sum=True)
    assert all(torch.is_tensor(v) and v.device.type == "cuda" for v in dev_out.values())
    assert dev_out["T"].shape == (6, 4, 4) and dev_out["trace"].shape == (6, 31, 2) and dev_out["w_sum"].shape == (6,)
    for name in ref:
        assert dev_out[name].cpu().numpy().tobytes() == ref[name].tobytes(), name
    # numpy in -> numpy out, torch on the host -> torch on the host; no trace or w_sum unless asked for
    for Tin in (T6, torch.from_numpy(T6)):
        out = colored_icp_refine(fo, O.SIX, Tin, 0.075)
        assert all((torch.is_tensor(v) and v.device.type == "cpu") if torch.is_tensor(Tin) else
                   isinstance(v, np.ndarray) for v in out.values()) and sorted(out) == sorted(NAMES[:-1])
        for name in out:
            assert np.asarray(out[name]).tobytes() == ref[name].tobytes(), name
    # what is missing is named
    bare = FragmentOverlap(O.scene4()[0][:2], "FCGF", 0.025, colors=CO.scene4_raw_colors()[:2])
    with pytest.raises(ValueError, match="normals"):
        colored_icp_refine(bare, [[0, 1]], T6[:1])
    with pytest.raises(ValueError, match="normals"):
        bare.compute_color_gradients()
    bare.estimate_normals()
    with pytest.raises(ValueError, match="intensity"):
        colored_icp_refine(bare, [[0, 1]], T6[:1])
    bare.intensity = fo.intensity[:bare.M].clone()
    with pytest.raises(ValueError, match="color_grad"):
        colored_icp_refine(bare, [[0, 1]], T6[:1])
    with pytest.raises(ValueError):
        bare.compute_color_gradients(radius=0.08)
    with pytest.raises(ValueError, match="colors"):
        FragmentOverlap(O.scene4()[0][:2], "FCGF", 0.025).compute_color_gradients()
    # a caller's own intensities and gradients: the two fragments' rows of the scene's
    bare.color_grad = fo.color_grad[:bare.M].clone()
    own = colored_icp_refine(bare, [[0, 1]], T6[:1], 0.075)
    assert own["T"].tobytes() == ref["T"][:1].tobytes()
    # colored_icp_pair: normals and gradients estimated there, on an index of cell max(max_dist, normal_radius)
    src, tgt, T_one, max_dist, iters = O.pair_case()
    sc, tc = CO.scene4_raw_colors()[0][4::8], CO.scene4_raw_colors()[1][4::8]
    one = colored_icp_pair(src, sc, tgt, tc, T_one, max_dist=max_dist, max_iters=iters, normal_radius=0.09)
    fo2 = FragmentOverlap([src, tgt], "3DMatch", radius=0.09, colors=[sc, tc])
    fo2.estimate_normals(0.09)
    fo2.compute_color_gradients(0.09)
    pts, nrm, I, g = _inputs(fo2)
    w = CO.colored_icp(pts[0], pts[1], nrm[1], I[0], I[1], g[1], T_one, max_dist, max_iters=iters)
    assert one["T"].shape == (4, 4) and int(one["n_corr"]) == w["n_corr"] and int(one["iters"]) == w["iters"]
    assert int(one["status"]) == w["status"]
    assert np.abs(one["T"][:3] - w["T"]).max() <= TOL and abs(one["rmse"] - w["rmse"]) <= TOL


# -------------------------------------------------------------------------------------------------------- scene chain
def test_register_scene_with_the_coloured_method(gpu):
    """plumbing: the refined estimates equal, bit for bit, colored_icp_refine called by hand on the result's fo"""
    from lib.icp import colored_icp_refine
    from lib.multiview import register_scene
    raw, colors = O.scene4()[0], CO.scene4_raw_colors()
    init = _six_starts()
    res = register_scene(raw, 0.025, method="colored", colors=colors, init=init, icp_lambda_geometric=0.9)
    fo, rec = res["fo"], res["pairs"]
    kept = rec["kept"]
    assert kept.sum() >= 3 and fo.colors is not None and fo.color_grad is not None
    assert fo.colors.cpu().numpy().tobytes() == _fo().colors.cpu().numpy().tobytes()
    ref = colored_icp_refine(fo, np.asarray(O.SIX)[kept], init[kept], lambda_geometric=0.9)
    assert rec["T"][kept].tobytes() == ref["T"].tobytes() and rec["fitness"][kept].tobytes() == ref["fitness"].tobytes()
    assert rec["T"][kept].tobytes() != colored_icp_refine(fo, np.asarray(O.SIX)[kept], init[kept])["T"].tobytes()
    with pytest.raises(ValueError, match="colors"):
        register_scene(raw, 0.025, method="colored", init=init)
    # colours with another method: carried along, nothing else changes
    other = register_scene(raw, 0.025, method="point_to_plane", colors=colors, init=init)
    plain = register_scene(raw, 0.025, method="point_to_plane", init=init)
    assert other["fo"].colors is not None and other["fo"].color_grad is None and plain["fo"].colors is None
    assert other["pairs"]["T"].tobytes() == plain["pairs"]["T"].tobytes()
    assert other["poses"].tobytes() == plain["poses"].tobytes()
