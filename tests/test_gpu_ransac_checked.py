"""GPU RANSAC with correspondence checkers (csrc/ransac.hip mvr_ransac_checked,
lib.utils.run_ransac_checked_batch, register_fpfh(checkers=...), register_scene(ransac_checkers=...)) against
mvr_ransac (checkers off: byte-identical) and the numpy restatement tests/ransac_checked_oracle.py:
  * the pass bits equal the oracle's on every iteration the oracle calls decided (no comparison within 1e-9 / 1e-7 of
    its threshold; test_ransac_checked_host.py caps their share at 1e-3 on these inputs, and finds none);
  * n_pass, n_valid and the validated list identical whenever no undecided iteration precedes the cap;
  * the exported hypotheses within 1e-9 of the oracle's LAPACK fits (Jacobi SVD vs LAPACK, as test_gpu_ransac.py);
  * best_iter, fitness and rmse bit-identical to the oracle's evaluation of the GPU's own hypotheses, T the winner's.
"""
import numpy as np
import pytest

import ransac_checked_oracle as C

pytestmark = pytest.mark.gpu
SENT = -77


def _gpu(x1, x2, counts, gpu, seed=C.SEED, ransac_n=3, iters=1000, max_dist=C.MAX_DIST, maxv=C.PARITY_CAP, edge=0.9,
         dist=C.MAX_DIST, n1=None, n2=None, ncos=-1.0):
    """mvr_ransac_checked on sentinel-filled outputs -> dict of numpy arrays (bits as bool [P, iters])"""
    import torch
    from lib import _native as N
    P, n = x1.shape[0], x1.shape[1]
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (x1, x2, n1, n2)]
    cnt = torch.tensor(counts, dtype=torch.int32, device=gpu)
    nw = (iters + 63) // 64
    f64 = lambda *s: torch.full(s, float(SENT), dtype=torch.float64, device=gpu)   # noqa: E731
    i32 = lambda *s: torch.full(s, SENT, dtype=torch.int32, device=gpu)            # noqa: E731
    o = {"T": f64(P, 4, 4), "fitness": f64(P), "rmse": f64(P), "best_iter": i32(P), "n_pass": i32(P),
         "n_valid": i32(P), "bits": torch.full((P, nw), SENT, dtype=torch.int64, device=gpu), "valid": i32(P, maxv),
         "hyp": f64(P, maxv, 12)}
    L = N.lib()
    ws = torch.empty(L.mvr_ransac_checked_workspace_bytes(P, iters, maxv), dtype=torch.uint8, device=gpu)
    rc = L.mvr_ransac_checked(N.ptr(dev[0]), N.ptr(dev[1]), n * 3, N.ptr(cnt), P, ransac_n, iters, max_dist, seed,
                              maxv, edge, dist, N.ptr(dev[2]), N.ptr(dev[3]), ncos, N.ptr(o["T"]), N.ptr(o["fitness"]),
                              N.ptr(o["rmse"]), N.ptr(o["best_iter"]), N.ptr(o["n_pass"]), N.ptr(o["n_valid"]),
                              N.ptr(o["bits"]), N.ptr(o["valid"]), N.ptr(o["hyp"]), N.ptr(ws), ws.numel(), N.stream())
    assert rc == 0
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in o.items()}
    words = o["bits"].view(np.uint64)
    o["words"] = words
    o["bits"] = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(P, -1)
    assert not o["bits"][:, iters:].any()          # the last word's bits past the iterations stay 0
    o["bits"] = o["bits"][:, :iters]
    return o


def _plain(x1, x2, counts, gpu, seed, ransac_n, iters):
    import torch
    from lib import _native as N
    P, n = x1.shape[0], x1.shape[1]
    X1, X2 = torch.from_numpy(x1).to(gpu), torch.from_numpy(x2).to(gpu)
    cnt = torch.tensor(counts, dtype=torch.int32, device=gpu)
    T = torch.empty(P, 4, 4, dtype=torch.float64, device=gpu)
    fit, rmse = (torch.empty(P, dtype=torch.float64, device=gpu) for _ in range(2))
    best = torch.empty(P, dtype=torch.int32, device=gpu)
    L = N.lib()
    ws = torch.empty(L.mvr_ransac_workspace_bytes(P, iters), dtype=torch.uint8, device=gpu)
    assert L.mvr_ransac(N.ptr(X1), N.ptr(X2), n * 3, N.ptr(cnt), P, ransac_n, iters, C.MAX_DIST, seed, N.ptr(T),
                        N.ptr(fit), N.ptr(rmse), N.ptr(best), None, N.ptr(ws), ws.numel(), N.stream()) == 0
    torch.cuda.synchronize()
    return {"T": T.cpu().numpy(), "fitness": fit.cpu().numpy(), "rmse": rmse.cpu().numpy(),
            "best_iter": best.cpu().numpy()}


def _compare(g, p, x1, x2, **kw):
    """pair p of the GPU result g against the oracle run with the same settings; returns the oracle's dict"""
    ref = C.ransac_checked(x1, x2, p=p, **kw)
    und = ref["undecided"]
    assert np.array_equal(g["bits"][p][~und], ref["bits"][~und]), (p, np.flatnonzero(g["bits"][p] != ref["bits"]))
    nv = int(g["n_valid"][p])
    maxv = kw["max_validation"]
    assert g["n_pass"][p] == g["bits"][p].sum() and nv == min(g["n_pass"][p], maxv)
    mine = np.flatnonzero(g["bits"][p])[:maxv]
    assert g["valid"][p, :nv].tolist() == mine.tolist() and (g["valid"][p, nv:] == -1).all()
    last = mine[-1] if nv == maxv else len(und)                 # iterations up to the cap
    if not und[:last + 1].any():
        assert g["n_valid"][p] == ref["n_valid"] and mine.tolist() == ref["valid"].tolist()
        if not und.any():
            assert g["n_pass"][p] == ref["n_pass"]
        if nv:   # the fits themselves, where the sample holds three distinct rows (else the rotation is not unique)
            idx = C.draws_all(kw["seed"], p, kw["iters"], kw.get("ransac_n", 3), len(x1))[mine]
            full = np.array([i for i in range(nv) if len(set(idx[i])) >= 3], dtype=np.int64)
            np.testing.assert_allclose(g["hyp"][p, :nv][full], ref["own"][full], rtol=0, atol=1e-9)
    # the selection over the GPU's own list and hypotheses, re-evaluated on the host: identical
    sel = C.ransac_checked(x1, x2, p=p, valid=mine, hyps=g["hyp"][p, :nv], **kw)
    assert g["best_iter"][p] == sel["best_iter"], (p, g["best_iter"][p], sel["best_iter"])
    assert g["fitness"][p] == sel["fitness"] and g["rmse"][p] == sel["rmse"]
    assert np.array_equal(g["T"][p], sel["T"])
    return ref


# ------------------------------------------------------------------------------------------------------- 1. anchor
@pytest.mark.parametrize("ransac_n", [3, 4])
@pytest.mark.parametrize("n,iters", [(300, 256), (37, 100)])
def test_checkers_off_is_mvr_ransac_byte_for_byte(gpu, n, iters, ransac_n):
    (x1, x2), counts = C.parity_inputs(n)
    counts = counts + [2]                                        # and a pair below ransac_n
    x1, x2 = np.concatenate([x1, x1[:1]]), np.concatenate([x2, x2[:1]])
    want = _plain(x1, x2, counts, gpu, C.SEED, ransac_n, iters)
    got = _gpu(x1, x2, counts, gpu, ransac_n=ransac_n, iters=iters, maxv=iters, edge=0.0, dist=0.0)
    for k in ("T", "fitness", "rmse", "best_iter"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["n_pass"].tolist() == [iters] * 3 + [0] and got["n_valid"].tolist() == [iters] * 3 + [0]
    assert (got["valid"][:3] == np.arange(iters)).all() and got["best_iter"][3] == -1
    more = _gpu(x1, x2, counts, gpu, ransac_n=ransac_n, iters=iters, maxv=iters + 77, edge=0.0, dist=0.0)
    for k in ("T", "fitness", "rmse", "best_iter"):
        assert more[k].tobytes() == want[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 2. oracle parity
@pytest.mark.parametrize("iters", C.PARITY_ITERS)
@pytest.mark.parametrize("n", C.PARITY_N)
def test_checkers_match_oracle(gpu, n, iters):
    (x1, x2), counts = C.parity_inputs(n)
    for mode, (edge, dist) in C.MODES.items():
        g = _gpu(x1, x2, counts, gpu, iters=iters, edge=edge, dist=dist)
        for p in range(3):
            m = counts[p]
            ref = _compare(g, p, x1[p, :m], x2[p, :m], seed=C.SEED, iters=iters, max_validation=C.PARITY_CAP,
                           edge_sim=edge, check_dist=dist)
            if m < 3:
                assert g["n_pass"][p] == 0 and g["best_iter"][p] == -1 and np.array_equal(g["T"][p], np.eye(4))
            if n == 1000 and iters == 4097:
                print("%s, inliers %.2f: %d of %d pass, best fitness %.3f" % (mode, (0.05, 0.3, 0.8)[p],
                                                                              ref["n_pass"], iters, ref["fitness"]))


# ---------------------------------------------------------------------------------------------------------- 3. cap
@pytest.mark.parametrize("cap", [1, 64])
def test_cap_validates_the_first_passing_iterations(gpu, cap):
    x1, x2, _, _ = C.corr(300, 0.8, seed=12)
    g = _gpu(x1[None], x2[None], [300], gpu, iters=1000, maxv=cap)
    full = _gpu(x1[None], x2[None], [300], gpu, iters=1000, maxv=1000)
    assert g["n_pass"][0] == full["n_pass"][0] > 64 and g["n_valid"][0] == cap
    assert g["words"].tobytes() == full["words"].tobytes()
    assert g["valid"][0].tolist() == np.flatnonzero(full["bits"][0])[:cap].tolist()
    assert g["best_iter"][0] in g["valid"][0]
    _compare(g, 0, x1, x2, seed=C.SEED, iters=1000, max_validation=cap, edge_sim=0.9, check_dist=C.MAX_DIST)
    if cap == 1:      # the one validated hypothesis is the result, whatever the uncapped run prefers
        assert g["best_iter"][0] == np.flatnonzero(full["bits"][0])[0] != full["best_iter"][0]


# --------------------------------------------------------------------------------------------------- 4. degenerate
def test_degenerate_inputs_write_every_row(gpu):
    x1, x2, _, _ = C.corr(64, 0.0, seed=3)                       # outliers only
    x1, x2 = np.stack([x1] * 4), np.stack([x2] * 4)
    x2[2, :3] = x1[2, :3] + 1.0                                  # pair 2: exactly three rows, a pure translation
    g = _gpu(x1, x2, [0, 2, 3, 64], gpu, iters=200, maxv=50, edge=0.999999)
    for k in ("T", "fitness", "rmse", "best_iter", "n_pass", "n_valid", "valid"):
        assert not (g[k] == SENT).any(), k
    assert not (g["words"] == np.uint64(SENT & (2**64 - 1))).any()
    for p in (0, 1, 3):        # n < ransac_n twice; 64 outliers whose edges never agree to 1e-6: nothing passes
        assert g["n_pass"][p] == g["n_valid"][p] == 0 and g["best_iter"][p] == -1 and not g["bits"][p].any()
        assert g["fitness"][p] == 0.0 and g["rmse"][p] == 0.0 and np.array_equal(g["T"][p], np.eye(4))
        assert (g["valid"][p] == -1).all()
    # n == ransac_n == 3: the samples of three distinct rows pass (6 of 27), and fit all three rows
    distinct = np.array([len(set(i)) == 3 for i in C.draws_all(C.SEED, 2, 200, 3, 3)])
    assert np.array_equal(g["bits"][2], distinct) and g["fitness"][2] == 1.0 and distinct[g["best_iter"][2]]
    np.testing.assert_allclose(g["T"][2], np.array([[1.0, 0, 0, 1], [0, 1, 0, 1], [0, 0, 1, 1], [0, 0, 0, 1]]),
                               atol=1e-9)
    _compare(g, 2, x1[2, :3], x2[2, :3], seed=C.SEED, iters=200, max_validation=50, edge_sim=0.999999,
             check_dist=C.MAX_DIST)


# ------------------------------------------------------------------------------------------------ 5. normal checker
def test_normal_checker_matches_oracle(gpu):
    (x1, x2, n1, n2), counts = C.parity_inputs(300, normals=True)
    ncos = float(np.cos(np.deg2rad(C.NORMAL_DEG)))
    g = _gpu(x1, x2, counts, gpu, iters=4097, n1=n1, n2=n2, ncos=ncos)
    off = _gpu(x1, x2, counts, gpu, iters=4097)
    only = _gpu(x1, x2, counts, gpu, iters=4097, n1=n1, n2=None, ncos=ncos)      # one array alone: checker off
    assert only["words"].tobytes() == off["words"].tobytes()
    for p in range(3):
        m = counts[p]
        _compare(g, p, x1[p, :m], x2[p, :m], seed=C.SEED, iters=4097, max_validation=C.PARITY_CAP, edge_sim=0.9,
                 check_dist=C.MAX_DIST, n1=n1[p, :m], n2=n2[p, :m], normal_cos=ncos)
        assert not (g["bits"][p] & ~off["bits"][p]).any()        # the normal check only removes
    # distance check off: samples with an outlier survive the edge check now and then, and their random normals
    # reject most of those
    ge = _gpu(x1, x2, counts, gpu, iters=4097, dist=0.0, n1=n1, n2=n2, ncos=ncos)
    oe = _gpu(x1, x2, counts, gpu, iters=4097, dist=0.0)
    assert ge["n_pass"][0] < oe["n_pass"][0]
    for p in range(3):
        m = counts[p]
        _compare(ge, p, x1[p, :m], x2[p, :m], seed=C.SEED, iters=4097, max_validation=C.PARITY_CAP, edge_sim=0.9,
                 check_dist=0.0, n1=n1[p, :m], n2=n2[p, :m], normal_cos=ncos)


# ----------------------------------------------------------------------------------------------- 6. reproducibility
def test_two_runs_are_byte_identical_and_batch_equals_single_calls(gpu):
    from lib.utils import run_ransac_checked_batch
    (x1, x2), counts = C.parity_inputs(1000)
    a = _gpu(x1, x2, counts, gpu, iters=4097)
    b = _gpu(x1, x2, counts, gpu, iters=4097)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    data = [C.corr(500, 0.25, seed=s) for s in range(4)]
    y1, y2 = np.stack([d[0] for d in data]), np.stack([d[1] for d in data])
    batch = run_ransac_checked_batch(y1, y2, seed=9, iters=3000, max_validation=300)
    assert set(batch) == {"T", "fitness", "rmse", "best_iter", "n_pass", "n_valid"}
    for p in range(4):
        # pair p of a batch draws from counter stream p; alone it draws from stream 0
        ref = C.ransac_checked(y1[p], y2[p], seed=9, iters=3000, max_validation=300, p=p)
        assert not ref["undecided"].any() and batch["n_pass"][p] == ref["n_pass"]
        assert batch["best_iter"][p] == ref["best_iter"] and abs(batch["fitness"][p] - ref["fitness"]) <= 2 / 500
        np.testing.assert_allclose(batch["T"][p], ref["T"], rtol=0, atol=1e-9)
        one = run_ransac_checked_batch(y1[p:p + 1], y2[p:p + 1], seed=9, iters=3000, max_validation=300)
        ref0 = C.ransac_checked(y1[p], y2[p], seed=9, iters=3000, max_validation=300, p=0)
        assert one["n_pass"][0] == ref0["n_pass"] and one["best_iter"][0] == ref0["best_iter"]
        np.testing.assert_allclose(one["T"][0], ref0["T"], rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------- 7. quality
def test_quality_case_recovers_planted_inliers_where_mvr_ransac_does_not(gpu):
    q = C.QUALITY
    x1, x2, R, t = C.corr(q["n"], q["inl"], q["data_seed"])
    g = _gpu(x1[None], x2[None], [q["n"]], gpu, seed=q["seed"], iters=q["iters"], maxv=q["max_validation"],
             edge=q["edge_sim"])
    ref = _compare(g, 0, x1, x2, seed=q["seed"], iters=q["iters"], max_validation=q["max_validation"],
                   edge_sim=q["edge_sim"], check_dist=C.MAX_DIST)
    # (the oracle's own LAPACK fits may count a borderline row differently: one row of slack on the fitness)
    assert not ref["undecided"].any() and g["best_iter"][0] == ref["best_iter"]
    assert abs(g["fitness"][0] - ref["fitness"]) <= 1 / q["n"]
    plain = _plain(x1[None], x2[None], [q["n"]], gpu, q["seed"], 4, 2500)
    print("checked: %d of %d samples pass, fitness %.4f (planted %.2f); mvr_ransac: fitness %.4f"
          % (g["n_pass"][0], q["iters"], g["fitness"][0], q["inl"], plain["fitness"][0]))
    assert g["fitness"][0] >= 0.9 * q["inl"] and plain["fitness"][0] < 0.5 * q["inl"]
    np.testing.assert_allclose(g["T"][0, :3, :3], R, atol=2e-2)
    np.testing.assert_allclose(g["T"][0, :3, 3], t, atol=3e-2)
    assert np.abs(plain["T"][0, :3, :3] - R).max() > 0.1


# ------------------------------------------------------------------------------------------------------ 8. end to end
def _rot_deg(Ra, Rb):
    return np.rad2deg(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def test_register_fpfh_with_checkers(gpu):
    """test_gpu_fpfh.py's full-copy case and its bounds (RANSAC_DIST at the centroid, 1 degree)"""
    import icp_oracle as IO
    from lib.fpfh import correspondences, match_features, register_fpfh
    from lib.overlap import FragmentOverlap
    from lib.utils import RANSAC_DIST, run_ransac_batch, run_ransac_checked_batch
    src = IO.scene4_centroids()[0]
    tgt, Tt, _ = IO.full_copy_case(src)
    c = src.mean(0)
    fo = FragmentOverlap([src, tgt], "3DMatch", radius=0.075)
    fo.estimate_normals(viewpoints=np.asarray([c, Tt[:3, :3] @ c + Tt[:3, 3]]))
    fo.compute_fpfh(0.075)
    out = register_fpfh(fo, [[0, 1]], seed=0, checkers=True)
    assert set(out) == {"T", "fitness", "rmse", "n_matches", "n_pass", "n_valid"} and out["T"].shape == (1, 4, 4)
    T = out["T"][0]
    dt = np.linalg.norm((T[:3, :3] @ c + T[:3, 3]) - (Tt[:3, :3] @ c + Tt[:3, 3]))
    dr = _rot_deg(T[:3, :3], Tt[:3, :3])
    print("register_fpfh(checkers): %d matches, %d of 100000 samples pass, %d scored, fitness %.3f; off by %.4f m, "
          "%.3f deg" % (out["n_matches"][0], out["n_pass"][0], out["n_valid"][0], out["fitness"][0], dt, dr))
    assert dt <= RANSAC_DIST and dr <= 1.0
    matches = match_features(fo.fpfh, fo.off, [[0, 1]])
    xs, xt = correspondences(fo, [[0, 1]], matches)
    by_hand = run_ransac_checked_batch(xs, xt, [len(matches[0])], seed=0)
    for k in ("T", "fitness", "rmse", "n_pass", "n_valid"):
        assert by_hand[k].tobytes() == out[k].tobytes(), k
    # overrides, the normal checker among them
    ns, nt = correspondences(fo, [[0, 1]], matches, fo.normals)
    opts = dict(iters=5000, max_validation=100, edge_sim=0.8, normal_deg=30.0)
    o2 = register_fpfh(fo, [[0, 1]], seed=3, checkers=opts)
    h2 = run_ransac_checked_batch(xs, xt, [len(matches[0])], seed=3, normals_i=ns, normals_j=nt, **opts)
    for k in ("T", "fitness", "rmse", "n_pass", "n_valid"):
        assert h2[k].tobytes() == o2[k].tobytes(), k
    assert o2["n_valid"][0] <= 100
    # the default call is what it was: run_ransac_batch's bytes, the four keys
    plain = register_fpfh(fo, [[0, 1]], seed=0)
    assert set(plain) == {"T", "fitness", "rmse", "n_matches"}
    assert plain["T"].tobytes() == run_ransac_batch(xs, xt, [len(matches[0])], seed=0).tobytes()
    assert register_fpfh(fo, [[0, 1]], seed=0, checkers=False)["T"].tobytes() == plain["T"].tobytes()
    empty = register_fpfh(fo, np.zeros((0, 2), np.int64), checkers=True)
    assert empty["T"].shape == (0, 4, 4) and len(empty["n_pass"]) == 0


def test_register_scene_with_checkers(gpu):
    """test_gpu_fuse.py's test_register_scene_weights_free with ransac_checkers=True, and its bounds"""
    import icp_oracle as IO
    from lib.multiview import register_scene
    from lib.utils import RANSAC_DIST
    src = IO.scene4_centroids()[0]
    c = src.mean(0)
    copies = [IO.full_copy_case(src, seed=s) for s in (3, 5)]
    frags = [src] + [cp[0] for cp in copies]
    truth = [np.eye(4)] + [np.linalg.inv(cp[1]) for cp in copies]
    views = np.asarray([c] + [cp[1][:3, :3] @ c + cp[1][:3, 3] for cp in copies])
    res = register_scene(frags, 0.025, viewpoints=views, downsample=False, seed=0, ransac_checkers=True)
    assert res["member"].tolist() == [1, 1, 1] and res["pairs"]["kept"][:2].all()
    for b in range(3):
        cb = views[b]
        M, G = res["poses"][b], truth[b]
        dt = np.linalg.norm((M[:3, :3] @ cb + M[:3, 3]) - (G[:3, :3] @ cb + G[:3, 3]))
        dr = _rot_deg(M[:3, :3], G[:3, :3])
        print("fragment %d: off by %.3g m at its centroid, %.3g deg" % (b, dt, dr))
        assert dt <= RANSAC_DIST and dr <= 1.0
