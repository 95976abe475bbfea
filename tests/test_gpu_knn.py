"""GPU k-nearest-neighbour search and outlier filters (csrc/knn_self.hip mvr_knn_self, csrc/outlier.hip
mvr_statistical_outlier / mvr_radius_count, lib.overlap.FragmentOverlap.knn / statistical_outliers / radius_outliers /
select, register_scene(denoise=...)) against the numpy oracle (tests/knn_oracle.py).

Tolerances.  idx and dist2 are a pure function of the points with every operation rounded on its own, so they must
equal the oracle's bit for bit; so must the masks and counts, whose cases keep every decision away from its threshold
(tests/test_knn_host.py asserts the margins).  mean_dist and threshold are fp64 sums of correctly rounded terms in
another order than numpy's pairwise sum, about 1e-15 relative: rtol 1e-12 leaves three orders of margin, and any
indexing error is at least a point spacing."""
import functools

import numpy as np
import pytest

import icp_oracle as O
import knn_oracle as K

pytestmark = pytest.mark.gpu
GUARD = 3          # rows of sentinels behind the outputs
S_IDX, S_D2 = -77, -77.0


def _raw(dev, frags, r, k):
    """mvr_radius_index_build + mvr_knn_self through the C ABI on sentinel-filled outputs -> (idx, dist2) as numpy;
    asserts that nothing behind the M k entries was written"""
    import torch
    from lib import _native as N
    L = N.lib()
    B = len(frags)
    off = K.offsets(frags)
    M = int(off[-1])
    xyz = torch.from_numpy(K.stack(frags)).to(dev)
    g_off = torch.from_numpy(off).to(dev)
    ib = L.mvr_radius_index_bytes(M)
    index = torch.empty(ib, dtype=torch.uint8, device=dev)
    assert L.mvr_radius_index_build(N.ptr(xyz), N.ptr(g_off), B, M, r, N.ptr(index), ib, N.stream()) == 0
    idx = torch.full((M + GUARD, k), S_IDX, dtype=torch.int32, device=dev)
    dist2 = torch.full((M + GUARD, k), S_D2, dtype=torch.float64, device=dev)
    ws_b = L.mvr_knn_self_workspace_bytes(M)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
    assert L.mvr_knn_self(N.ptr(index), ib, N.ptr(xyz), N.ptr(g_off), B, M, r, k, N.ptr(idx), N.ptr(dist2), N.ptr(ws),
                          ws_b, N.stream()) == 0
    assert (idx[M:] == S_IDX).all() and (dist2[M:] == S_D2).all()
    scanned = int(ws[:4].view(torch.int32).item())
    return idx[:M].cpu().numpy(), dist2[:M].cpu().numpy(), scanned


def _same(what, got_idx, got_d2, want_idx, want_d2):
    assert got_idx.shape == want_idx.shape and got_idx.dtype == np.int32 and got_d2.dtype == np.float64
    bad = np.flatnonzero((got_idx != want_idx).any(1) | (got_d2.view(np.int64) != want_d2.view(np.int64)).any(1))
    assert len(bad) == 0, (what, len(bad), bad[:5], got_idx[bad[:2]], want_idx[bad[:2]])


# ------------------------------------------------------------------------------------------------------ mvr_knn_self
@pytest.mark.parametrize("k", [1, 8, 20, 64])
def test_two_clouds_match_the_oracle_bit_for_bit(gpu, k):
    A, B = K.clouds()[:2]
    want_idx, want_d2 = K.clouds_knn(k)
    idx, d2, scanned = _raw(gpu, [A, B], K.R_CELL, k)
    ring = K.resolving_ring(K.stack([A, B]), K.offsets([A, B]), k, K.R_CELL)
    print("k = %d: %d of %d queries went to the direct scan (the rule predicts %d)"
          % (k, scanned, len(idx), (ring == 0).sum()))
    _same("clouds, k = %d" % k, idx, d2, want_idx, want_d2)
    assert (idx >= 0).all() and np.isfinite(d2).all() and 0 <= scanned <= len(idx)


def test_ragged_fragments_are_padded_and_fully_written(gpu):
    frags = K.ragged_case()
    off = K.offsets(frags)
    want_idx, want_d2 = K.knn_self(K.stack(frags), off, 20)
    idx, d2, _ = _raw(gpu, frags, K.R_CELL, 20)
    _same("ragged", idx, d2, want_idx, want_d2)                              # no sentinel is left: all written
    for b, n in enumerate(np.diff(off)):
        rows = slice(off[b], off[b + 1])
        assert (idx[rows, :min(n, 20)] >= off[b]).all() and (idx[rows, :min(n, 20)] < off[b + 1]).all()
        assert (idx[rows, min(n, 20):] == -1).all() and np.isposinf(d2[rows, min(n, 20):]).all()


def test_sparse_cloud_takes_the_direct_scan(gpu):
    frags, r, k = K.sparse_case()
    want_idx, want_d2 = K.knn_self(K.stack(frags), K.offsets(frags), k)
    idx, d2, scanned = _raw(gpu, frags, r, k)
    print("sparse: %d of %d queries went to the direct scan" % (scanned, len(idx)))
    _same("sparse", idx, d2, want_idx, want_d2)
    assert scanned > 0.9 * len(idx)


def test_isolated_points_are_exact(gpu):
    frags = K.isolated_case()
    want_idx, want_d2 = K.knn_self(K.stack(frags), K.offsets(frags), 20)
    idx, d2, scanned = _raw(gpu, frags, K.R_CELL, 20)
    _same("isolated", idx, d2, want_idx, want_d2)
    assert scanned >= 5 and (np.sqrt(d2[-5:, 1]) > 0.5).all()


def test_ties_and_cell_faces_come_lower_row_first(gpu):
    frags, r = K.ties_case()
    want_idx, want_d2 = K.knn_self(K.stack(frags), K.offsets(frags), 20)
    idx, d2, _ = _raw(gpu, frags, r, 20)
    _same("ties", idx, d2, want_idx, want_d2)


def test_a_fragment_does_not_depend_on_the_batch_and_runs_repeat(gpu):
    A, B = K.clouds()[:2]
    small = K.ragged_case()[5]
    alone = _raw(gpu, [B], K.R_CELL, 20)
    third = _raw(gpu, [A, small, B], K.R_CELL, 20)
    o = len(A) + len(small)
    assert alone[1].tobytes() == third[1][o:].tobytes()
    np.testing.assert_array_equal(alone[0], third[0][o:] - o)
    again = _raw(gpu, [A, small, B], K.R_CELL, 20)
    assert again[0].tobytes() == third[0].tobytes() and again[1].tobytes() == third[1].tobytes()


def test_arguments_on_the_device(gpu):
    import torch
    from lib import _native as N
    L = N.lib()
    z, s = None, N.stream()
    x = torch.zeros(10, 3, dtype=torch.float64, device=gpu)
    off = torch.tensor([0, 10], dtype=torch.int64, device=gpu)
    ib = L.mvr_radius_index_bytes(10)
    index = torch.empty(ib, dtype=torch.uint8, device=gpu)
    assert L.mvr_radius_index_build(N.ptr(x), N.ptr(off), 1, 10, 0.05, N.ptr(index), ib, s) == 0
    idx = torch.empty(10, 4, dtype=torch.int32, device=gpu)
    d2 = torch.empty(10, 4, dtype=torch.float64, device=gpu)
    ws_b = L.mvr_knn_self_workspace_bytes(10)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=gpu)
    good = [N.ptr(index), ib, N.ptr(x), N.ptr(off), 1, 10, 0.05, 4, N.ptr(idx), N.ptr(d2), N.ptr(ws), ws_b, s]
    assert L.mvr_knn_self(*good) == 0
    assert idx.cpu().numpy().tolist() == [[0, 1, 2, 3]] * 10 and not d2.any()        # ten coincident points
    for at in (0, 2, 3, 8, 9, 10):
        args = list(good)
        args[at] = z
        assert L.mvr_knn_self(*args) == -1, at
    for at, v in ((1, ib - 1), (11, ws_b - 1), (7, 0), (7, 65), (6, 0.0)):
        args = list(good)
        args[at] = v
        assert L.mvr_knn_self(*args) == -1, at
    keep = torch.empty(10, dtype=torch.uint8, device=gpu)
    mean = torch.empty(10, dtype=torch.float64, device=gpu)
    thr = torch.empty(1, dtype=torch.float64, device=gpu)
    good = [N.ptr(d2), N.ptr(off), 1, 10, 4, 2.0, N.ptr(keep), N.ptr(mean), N.ptr(thr), s]
    assert L.mvr_statistical_outlier(*good) == 0
    assert not mean.any() and thr.item() == 0.0 and not keep.any()                   # 0 < 0 is false: strict
    for at in (0, 1, 6, 7, 8):
        args = list(good)
        args[at] = z
        assert L.mvr_statistical_outlier(*args) == -1, at
    cnt = torch.empty(10, dtype=torch.int32, device=gpu)
    good = [N.ptr(index), ib, N.ptr(x), N.ptr(off), 1, 10, 0.05, 0.05, N.ptr(cnt), s]
    assert L.mvr_radius_count(*good) == 0 and (cnt == 10).all()
    for at in (0, 2, 3, 8):
        args = list(good)
        args[at] = z
        assert L.mvr_radius_count(*args) == -1, at
    args = list(good)
    args[1] = ib - 1
    assert L.mvr_radius_count(*args) == -1


# ------------------------------------------------------------------------------------------------- FragmentOverlap
@functools.lru_cache(maxsize=None)
def _clouds_fo():
    from lib.overlap import FragmentOverlap
    return FragmentOverlap(list(K.clouds()[:2]), "3DMatch", radius=K.R_CELL)


def test_fo_knn_and_the_two_filters_match_the_oracle(gpu):
    import torch
    fo = _clouds_fo()
    A, B, pa, pb = K.clouds()
    planted = np.concatenate([pa, pb])
    off = K.offsets([A, B])
    idx, d2 = fo.knn(K.K_STAT)
    assert idx.device == fo.xyz.device and idx.dtype == torch.int32 and d2.dtype == torch.float64
    want_idx, want_d2 = K.clouds_knn(K.K_STAT)
    _same("fo.knn", idx.cpu().numpy(), d2.cpu().numpy(), want_idx, want_d2)
    want = K.statistical(want_d2, off, K.K_STAT, K.STD_RATIO)
    got = fo.statistical_outliers()
    assert set(got) == {"keep", "mean_dist", "threshold"} and got["keep"].dtype == torch.bool
    assert got["keep"].device == fo.xyz.device and tuple(got["threshold"].shape) == (2,)
    np.testing.assert_array_equal(got["keep"].cpu().numpy(), want["keep"])
    np.testing.assert_allclose(got["mean_dist"].cpu().numpy(), want["mean_dist"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["threshold"].cpu().numpy(), want["threshold"], rtol=1e-12, atol=0)
    assert not want["keep"][planted].any() and want["keep"][~planted].all()
    again = fo.statistical_outliers(K.K_STAT, K.STD_RATIO)                           # fixed order: the same bits
    for key in got:
        assert again[key].cpu().numpy().tobytes() == got[key].cpu().numpy().tobytes(), key
    count = K.radius_count(fo.xyz.cpu().numpy(), off, K.R_CELL)
    got = fo.radius_outliers(K.NB_POINTS)
    assert set(got) == {"keep", "count"} and got["count"].dtype == torch.int32 and got["keep"].dtype == torch.bool
    np.testing.assert_array_equal(got["count"].cpu().numpy(), count)
    np.testing.assert_array_equal(got["keep"].cpu().numpy(), count > K.NB_POINTS)
    np.testing.assert_array_equal(got["keep"].cpu().numpy(), ~planted)
    half = fo.radius_outliers(K.NB_POINTS, 0.04)
    np.testing.assert_array_equal(half["count"].cpu().numpy(), K.radius_count(fo.xyz.cpu().numpy(), off, 0.04))
    fo.estimate_normals()
    np.testing.assert_array_equal(fo.n_nbr.cpu().numpy(), count)                     # the walk the normals take
    with pytest.raises(ValueError, match="must lie in"):
        fo.radius_outliers(8, 0.08)
    with pytest.raises(ValueError):
        fo.statistical_outliers(65)
    with pytest.raises(ValueError):
        fo.knn(0)


def test_select_keeps_rows_in_order_and_rebuilds_the_index(gpu):
    import torch
    from lib.overlap import FragmentOverlap
    fo = _clouds_fo()
    keep = fo.statistical_outliers()["keep"]
    fo2 = fo.select(keep)
    k_np = keep.cpu().numpy()
    off = K.offsets(K.clouds()[:2])
    assert isinstance(fo2, FragmentOverlap) and fo2.M == k_np.sum() == fo.M - 60 and fo2.B == 2
    assert (fo2.method, fo2.voxel_size, fo2.r, fo2.device) == (fo.method, fo.voxel_size, fo.r, fo.device)
    assert fo2.xyz.cpu().numpy().tobytes() == fo.xyz.cpu().numpy()[k_np].tobytes()
    want_off = [0, int(k_np[:off[1]].sum()), int(k_np.sum())]
    assert fo2.off.tolist() == want_off and fo2.off_dev.cpu().tolist() == want_off and fo2.off.dtype == np.int64
    assert fo2.max_points == max(np.diff(want_off))
    assert fo2.parent_rows.dtype == torch.int64 and fo2.parent_rows.cpu().tolist() == np.flatnonzero(k_np).tolist()
    assert fo2.normals is None and fo2.n_nbr is None and fo2.fpfh is None
    pts = fo2.xyz.cpu().numpy()
    idx, d2 = fo2.knn(20)
    want = K.knn_self(pts, fo2.off, 20)
    _same("select, knn", idx.cpu().numpy(), d2.cpu().numpy(), *want)
    fo2.estimate_normals()
    count, margin = K.radius_count(pts, fo2.off, fo2.r, with_margin=True)
    assert margin > 1e-9
    np.testing.assert_array_equal(fo2.n_nbr.cpu().numpy(), count)
    # numpy uint8 masks do; one fragment emptied: the calls above accept it
    mask = np.ones(fo.M, np.uint8)
    mask[:off[1]] = 0
    fo3 = fo.select(mask)
    assert fo3.off.tolist() == [0, 0, int(off[2] - off[1])] and fo3.M == off[2] - off[1]
    assert fo3.xyz.cpu().numpy().tobytes() == fo.xyz.cpu().numpy()[off[1]:].tobytes()
    idx, d2 = fo3.knn(20)
    want = K.knn_self(fo3.xyz.cpu().numpy(), fo3.off, 20)
    _same("select, one fragment emptied", idx.cpu().numpy(), d2.cpu().numpy(), *want)
    st = fo3.statistical_outliers()
    assert np.isposinf(st["threshold"][0].item()) and np.isfinite(st["threshold"][1].item())
    assert fo3.radius_outliers(8)["count"].shape == (fo3.M,) and fo3.estimate_normals().shape == (fo3.M, 3)
    fo4 = fo3.select(torch.zeros(fo3.M, dtype=torch.bool, device=gpu))               # nothing left at all
    assert fo4.M == 0 and fo4.off.tolist() == [0, 0, 0] and tuple(fo4.knn(3)[0].shape) == (0, 3)
    assert fo4.statistical_outliers()["keep"].shape == (0,) and fo4.radius_outliers()["count"].shape == (0,)
    with pytest.raises(ValueError, match="select: keep"):
        fo.select(np.ones(fo.M - 1, bool))
    with pytest.raises(ValueError, match="select: keep"):
        fo.select(np.ones(fo.M, np.int64))


# ---------------------------------------------------------------------------------------------------- register_scene
def _oracle_removed(fo):
    """per fragment the points the statistical filter removes from fo's centroids, by the oracle"""
    _, d2 = K.knn_self(fo.xyz.cpu().numpy(), fo.off, K.K_STAT)
    keep = K.statistical(d2, fo.off, K.K_STAT, K.STD_RATIO)["keep"]
    return keep, np.asarray([(~keep[fo.off[b]:fo.off[b + 1]]).sum() for b in range(fo.B)])


def test_register_scene_denoise_is_the_chain_on_the_kept_points(gpu):
    from lib.icp import icp_refine, information_matrix
    from lib.multiview import fuse_scene, optimize_pose_graph, register_scene, synchronize
    from lib.overlap import FragmentOverlap
    frags, flying = K.scene_case()
    init = O.scene4_starts(O.SIX, O.scene4_centroids())
    spec = {"method": "statistical", "nb_neighbors": K.K_STAT, "std_ratio": K.STD_RATIO}
    res = register_scene(frags, 0.025, init=init, method="point_to_plane", denoise=spec)
    pairs = np.asarray(O.SIX)
    full = FragmentOverlap(frags, "FCGF", 0.025)
    want_keep, want_removed = _oracle_removed(full)
    print("denoise removed %s points of %s" % (res["denoise"]["removed"].tolist(), np.diff(full.off).tolist()))
    assert set(res["denoise"]) == {"keep", "removed"} and res["denoise"]["keep"].dtype == bool
    np.testing.assert_array_equal(res["denoise"]["keep"], want_keep)
    np.testing.assert_array_equal(res["denoise"]["removed"], want_removed)
    assert (want_removed >= K.N_SCENE_PLANTED).all()
    fo = full.select(want_keep)
    assert res["fo"].xyz.cpu().numpy().tobytes() == fo.xyz.cpu().numpy().tobytes()
    assert res["fo"].off.tolist() == fo.off.tolist()
    fo.estimate_normals(None, np.zeros((4, 3)))
    overlap = fo.ratios(pairs, np.linalg.inv(init))
    kept = overlap >= 0.3
    ref = icp_refine(fo, pairs[kept], init[kept], method="point_to_plane")
    info = information_matrix(fo, pairs[kept], ref["T"])
    sync = synchronize(ref["T"][:, :3, :3], ref["T"][:, :3, 3], pairs[kept], 4, irls_iters=5)
    pg = optimize_pose_graph(sync["R"], sync["t"], ref["T"][:, :3, :3], ref["T"][:, :3, 3], pairs[kept],
                             info["info"], sync["weights"])
    scene = fuse_scene(fo, pg["R"], pg["t"], 0.025, member=pg["member"])
    rec = res["pairs"]
    assert kept.sum() >= 3 and rec["kept"].tolist() == kept.tolist() and rec["overlap"].tobytes() == overlap.tobytes()
    assert rec["T"][kept].tobytes() == ref["T"].tobytes()
    assert res["R"].tobytes() == pg["R"].tobytes() and res["t"].tobytes() == pg["t"].tobytes()
    for k in ("xyz", "normals", "n_points", "n_frags"):
        assert res["scene"][k].cpu().numpy().tobytes() == scene[k].cpu().numpy().tobytes(), k
    # no fused point within half a voxel of a flying pixel's place in the scene
    fused = res["scene"]["xyz"].cpu().numpy()
    assert res["scene"]["n_points"].sum().item() == fo.M and len(fused) > 100
    for b, p in enumerate(flying):
        mapped = p.astype(np.float64) @ res["R"][b].T + res["t"][b]
        d = np.sqrt(((fused[:, None, :] - mapped[None]) ** 2).sum(2)).min(0)
        assert d.min() > 0.0125, (b, d.min())


def test_register_scene_denoise_none_and_radius(gpu):
    from lib.multiview import register_scene
    from lib.overlap import FragmentOverlap
    frags = K.scene_case()[0]
    init = O.scene4_starts(O.SIX, O.scene4_centroids())
    # denoise=None is the call without the argument
    clean = O.scene4()[0]
    a = register_scene(clean, 0.025, init=init, method="point_to_plane", denoise=None)
    b = register_scene(clean, 0.025, init=init, method="point_to_plane")
    assert set(a) == set(b) and "denoise" not in a
    assert a["poses"].tobytes() == b["poses"].tobytes() and a["pairs"]["T"].tobytes() == b["pairs"]["T"].tobytes()
    for k in ("xyz", "normals", "n_points", "n_frags"):
        assert a["scene"][k].cpu().numpy().tobytes() == b["scene"][k].cpu().numpy().tobytes(), k
    # the radius filter through the same argument
    rad = register_scene(frags, 0.025, init=init, denoise={"method": "radius", "nb_points": 4})
    full = FragmentOverlap(frags, "FCGF", 0.025)
    count, margin = K.radius_count(full.xyz.cpu().numpy(), full.off, full.r, with_margin=True)
    assert margin > 1e-9
    np.testing.assert_array_equal(rad["denoise"]["keep"], count > 4)
    assert rad["fo"].M == (count > 4).sum() and rad["denoise"]["removed"].sum() == (count <= 4).sum()


def test_register_scene_cli_denoise_writes_what_register_scene_returns(gpu, tmp_path, capsys):
    from lib.multiview import register_scene
    from lib.ply import read_ply_xyz, write_ply_xyz
    from lib.utils import write_trajectory
    from scripts.fuse_scene import read_poses
    from scripts.register_scene import main, read_init
    frags = K.scene_case()[0]
    files = []
    for b, f in enumerate(frags):
        files.append(str(tmp_path / ("frag_%d.ply" % b)))
        write_ply_xyz(files[-1], f)
    start = O.scene4_starts(O.SIX, O.scene4_centroids())
    write_trajectory(np.linalg.inv(start), [[i, j, True] for i, j in O.SIX], str(tmp_path / "init.txt"))
    out = str(tmp_path / "out")
    main(["--fragments"] + files + ["--out", out, "--init", str(tmp_path / "init.txt"), "--denoise",
                                    "statistical:20:2.0"])
    want = register_scene([read_ply_xyz(f) for f in files], 0.025, init=read_init(str(tmp_path / "init.txt"), 4),
                          denoise={"method": "statistical", "nb_neighbors": 20, "std_ratio": 2.0})
    printed = capsys.readouterr().out
    assert "registered 4 fragments" in printed
    assert ("denoise (statistical): points removed per fragment: %s"
            % " ".join(str(int(v)) for v in want["denoise"]["removed"])) in printed
    assert (want["denoise"]["removed"] >= K.N_SCENE_PLANTED).all()
    np.testing.assert_allclose(read_poses(out + "/poses.txt", 4), want["poses"], rtol=0, atol=1e-11)
    blob = open(out + "/scene.ply", "rb").read()
    rows = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], "<f4").reshape(-1, 6)
    assert len(rows) > 100 and rows[:, :3].tobytes() == want["scene"]["xyz"].cpu().numpy().astype("<f4").tobytes()
    assert rows[:, 3:].tobytes() == want["scene"]["normals"].cpu().numpy().astype("<f4").tobytes()
