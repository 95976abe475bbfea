"""GPU DBSCAN clustering (csrc/dbscan.hip mvr_cluster_dbscan, lib.overlap.FragmentOverlap.cluster_dbscan /
cluster_keep, register_scene(denoise={"method": "cluster", ...})) against the numpy oracle (tests/dbscan_oracle.py),
which restates Open3D's sequential loop and shares nothing with the kernels' union-find.

Tolerances: none.  labels, n_clusters, sizes and core are integers decided by comparisons of a distance with eps, and
every case keeps every distance away from eps by more than 1e-9 relative (tests/test_dbscan_host.py asserts it on the
oracle), far above the rounding of the distance under any contraction; so they must equal the oracle's exactly."""
import functools

import numpy as np
import pytest

import dbscan_oracle as D
import icp_oracle as O
import knn_oracle as K

pytestmark = pytest.mark.gpu
GUARD = 3          # rows of sentinels behind the outputs
S_LAB, S_CNT, S_SIZE, S_CORE = -77, -78, -79, 77


def _raw(dev, frags, r, eps, min_points, sizes=True, core=True):
    """mvr_radius_index_build + mvr_cluster_dbscan through the C ABI on sentinel-filled outputs -> dict of numpy
    arrays (sizes / core None where they were not asked for); asserts that nothing behind M (or B) was written"""
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
    labels = torch.full((M + GUARD,), S_LAB, dtype=torch.int32, device=dev)
    n_clusters = torch.full((B + GUARD,), S_CNT, dtype=torch.int32, device=dev)
    g_sizes = torch.full((M + GUARD,), S_SIZE, dtype=torch.int32, device=dev) if sizes else None
    g_core = torch.full((M + GUARD,), S_CORE, dtype=torch.uint8, device=dev) if core else None
    ws_b = L.mvr_dbscan_workspace_bytes(M)
    ws = torch.full((ws_b + 256,), 0x5A, dtype=torch.uint8, device=dev)
    assert L.mvr_cluster_dbscan(N.ptr(index), ib, N.ptr(xyz), N.ptr(g_off), B, M, r, eps, min_points, N.ptr(labels),
                                N.ptr(n_clusters), N.ptr(g_sizes), N.ptr(g_core), N.ptr(ws), ws_b, N.stream()) == 0
    assert (labels[M:] == S_LAB).all() and (n_clusters[B:] == S_CNT).all() and (ws[ws_b:] == 0x5A).all()
    out = {"labels": labels[:M].cpu().numpy(), "n_clusters": n_clusters[:B].cpu().numpy(), "sizes": None,
           "core": None}
    if sizes:
        assert (g_sizes[M:] == S_SIZE).all()
        out["sizes"] = g_sizes[:M].cpu().numpy()
    if core:
        assert (g_core[M:] == S_CORE).all()
        out["core"] = g_core[:M].cpu().numpy()
    return out


def _same(what, got, want):
    assert got["labels"].dtype == np.int32 and got["n_clusters"].dtype == np.int32
    bad = np.flatnonzero(got["labels"] != want["labels"])
    assert len(bad) == 0, (what, "labels", len(bad), bad[:5], got["labels"][bad[:5]], want["labels"][bad[:5]])
    np.testing.assert_array_equal(got["n_clusters"], want["n_clusters"], err_msg=what)
    if got["sizes"] is not None:
        np.testing.assert_array_equal(got["sizes"], want["sizes"], err_msg=what)       # no sentinel is left either
    if got["core"] is not None:
        np.testing.assert_array_equal(got["core"], want["core"].astype(np.uint8), err_msg=what)


# ------------------------------------------------------------------------------------------------ mvr_cluster_dbscan
@pytest.mark.parametrize("name", ["clouds", "blobs", "helices", "ties", "ragged"])
def test_cases_match_the_oracle_exactly(gpu, name):
    frags, r, eps, min_points = D.CASES[name]()
    want = D.case_oracle(name)[2]
    got = _raw(gpu, frags, r, eps, min_points)
    print("%s: clusters %s, %d noise, %d core" % (name, got["n_clusters"].tolist(), (got["labels"] < 0).sum(),
                                                  got["core"].sum()))
    _same(name, got, want)


def test_a_fragment_does_not_depend_on_the_batch(gpu):
    A, B = K.clouds()[:2]
    small = K.ragged_case()[5]
    _, r, eps, min_points = D.clouds_case()
    alone = _raw(gpu, [B], r, eps, min_points)
    third = _raw(gpu, [A, small, B], r, eps, min_points)
    o = len(A) + len(small)
    for key in ("labels", "sizes", "core"):                                  # labels are per fragment: no offset
        assert alone[key].tobytes() == third[key][o:].tobytes(), key
    assert alone["n_clusters"][0] == third["n_clusters"][2]
    off = K.offsets([A, small, B])
    _same("[A, small, B]", third, D.dbscan(K.stack([A, small, B]), off, eps, min_points))


@pytest.mark.parametrize("name", ["helices", "blobs"])
def test_runs_repeat_byte_for_byte(gpu, name):
    frags, r, eps, min_points = D.CASES[name]()
    first = _raw(gpu, frags, r, eps, min_points)
    again = _raw(gpu, frags, r, eps, min_points)
    for key in ("labels", "n_clusters", "sizes", "core"):                    # the hooking's interleaving stays inside
        assert first[key].tobytes() == again[key].tobytes(), key


def test_min_points_one_and_eps_equal_to_the_cell(gpu):
    A, B = K.clouds()[:2]
    got = _raw(gpu, [A, B], K.R_CELL, 0.05, 1)
    assert got["core"].all() and (got["labels"] >= 0).all()
    off = K.offsets([A, B])
    _same("min_points = 1", got, D.dbscan(K.stack([A, B]), off, 0.05, 1))
    assert D.margin(K.stack([A, B]), off, K.R_CELL) > 1e-9
    got = _raw(gpu, [A, B], K.R_CELL, K.R_CELL, 8)                           # eps == r_index exactly is accepted
    _same("eps = cell", got, D.dbscan(K.stack([A, B]), off, K.R_CELL, 8))


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
    labels = torch.full((10,), S_LAB, dtype=torch.int32, device=gpu)
    n_clusters = torch.full((1,), S_CNT, dtype=torch.int32, device=gpu)
    sizes = torch.full((10,), S_SIZE, dtype=torch.int32, device=gpu)
    core = torch.full((10,), S_CORE, dtype=torch.uint8, device=gpu)
    ws_b = L.mvr_dbscan_workspace_bytes(10)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=gpu)
    good = [N.ptr(index), ib, N.ptr(x), N.ptr(off), 1, 10, 0.05, 0.05, 10, N.ptr(labels), N.ptr(n_clusters),
            N.ptr(sizes), N.ptr(core), N.ptr(ws), ws_b, s]
    assert L.mvr_cluster_dbscan(*good) == 0
    assert labels.tolist() == [0] * 10 and n_clusters.tolist() == [1] and sizes.tolist() == [10] + [0] * 9
    assert core.tolist() == [1] * 10                                         # ten coincident points, min_points 10
    args = list(good)
    args[8] = 11
    assert L.mvr_cluster_dbscan(*args) == 0 and labels.tolist() == [-1] * 10 and n_clusters.tolist() == [0]
    assert not sizes.any() and not core.any()
    for at in (0, 2, 3, 9, 10, 13):                                          # NULL index, xyz, off, labels, ...
        args = list(good)
        args[at] = z
        assert L.mvr_cluster_dbscan(*args) == -1, at
    for at, v in ((1, ib - 1), (14, ws_b - 1), (8, 0), (7, 0.0500001), (7, 0.0), (6, 0.0)):
        args = list(good)
        args[at] = v
        assert L.mvr_cluster_dbscan(*args) == -1, at
    for at in (11, 12):                                                      # NULL sizes or NULL core is accepted
        labels.fill_(S_LAB)
        args = list(good)
        args[at] = z
        assert L.mvr_cluster_dbscan(*args) == 0 and labels.tolist() == [0] * 10, at
    frags, r, eps, min_points = D.blobs_case()
    want = D.case_oracle("blobs")[2]
    _same("blobs without sizes", _raw(gpu, frags, r, eps, min_points, sizes=False), want)
    _same("blobs without core", _raw(gpu, frags, r, eps, min_points, core=False), want)


# ------------------------------------------------------------------------------------------------- FragmentOverlap
def test_fo_cluster_dbscan_and_cluster_keep_match_the_oracle(gpu):
    import torch
    from lib.overlap import FragmentOverlap
    frags, r, eps, min_points = D.blobs_case()
    empty = np.zeros((0, 3))
    lone = np.array([[3.0, 3.0, 3.0]])
    fo = FragmentOverlap([frags[0], empty, lone, frags[0][:700]], "3DMatch", radius=r)
    xyz, off = fo.xyz.cpu().numpy(), fo.off
    want = D.dbscan(xyz, off, eps, min_points)
    got = fo.cluster_dbscan(eps, min_points)
    assert set(got) == {"labels", "n_clusters", "sizes", "core"}
    assert got["labels"].dtype == torch.int32 and got["sizes"].dtype == torch.int32 and got["core"].dtype == torch.bool
    for key in ("labels", "sizes", "core"):
        assert got[key].device == fo.xyz.device and tuple(got[key].shape) == (fo.M,)
        np.testing.assert_array_equal(got[key].cpu().numpy(), want[key], err_msg=key)
    assert isinstance(got["n_clusters"], np.ndarray) and got["n_clusters"].dtype == np.int64
    assert got["n_clusters"].tolist() == want["n_clusters"].tolist() and got["n_clusters"][1:3].tolist() == [0, 0]
    for min_size in (1, 60, 120, 10 ** 6):
        keep = fo.cluster_keep(got, min_size=min_size)
        assert keep.dtype == torch.bool and keep.device == fo.xyz.device and tuple(keep.shape) == (fo.M,)
        np.testing.assert_array_equal(keep.cpu().numpy(), D.cluster_keep(want, off, min_size=min_size))
    assert 0 < fo.cluster_keep(got, min_size=60).sum().item() < (got["labels"] >= 0).sum().item()
    largest = fo.cluster_keep(got, largest=True).cpu().numpy()
    np.testing.assert_array_equal(largest, D.cluster_keep(want, off, largest=True))
    assert largest[:off[1]].sum() == want["sizes"][:off[1]].max() and not largest[off[1]:off[3]].any()
    # eps None is the index's cell; the mask goes through select
    whole = fo.cluster_dbscan(None, min_points)
    np.testing.assert_array_equal(whole["labels"].cpu().numpy(), D.dbscan(xyz, off, r, min_points)["labels"])
    assert D.margin(xyz, off, r) > 1e-9
    fo2 = fo.select(fo.cluster_keep(got, largest=True))
    assert fo2.M == largest.sum() and fo2.off.tolist() == [0] + np.cumsum([largest[off[b]:off[b + 1]].sum()
                                                                          for b in range(4)]).tolist()
    with pytest.raises(ValueError, match="cluster_dbscan: eps"):
        fo.cluster_dbscan(r * 1.01)
    with pytest.raises(ValueError, match="cluster_keep"):
        fo.cluster_keep(got)
    nothing = fo.select(torch.zeros(fo.M, dtype=torch.bool, device=gpu))
    none = nothing.cluster_dbscan()
    assert none["labels"].shape == (0,) and none["n_clusters"].tolist() == [0, 0, 0, 0]
    assert nothing.cluster_keep(none, min_size=1).shape == (0,)


def test_a_tie_for_the_largest_cluster_keeps_the_lower_number(gpu):
    from lib.overlap import FragmentOverlap
    pts = np.array([[0.0, 0, 0], [0.01, 0, 0], [0.5, 0, 0], [0.51, 0, 0], [0.9, 0, 0]])
    fo = FragmentOverlap([pts, pts[2:]], "3DMatch", radius=0.05)
    got = fo.cluster_dbscan(0.02, 2)
    assert got["labels"].tolist() == [0, 0, 1, 1, -1, 0, 0, -1] and got["n_clusters"].tolist() == [2, 1]
    assert fo.cluster_keep(got, largest=True).tolist() == [True, True, False, False, False, True, True, False]
    assert fo.cluster_keep(got, min_size=2).tolist() == [True] * 4 + [False, True, True, False]


# ---------------------------------------------------------------------------------------------------- register_scene
@functools.lru_cache(maxsize=None)
def _scene_oracle():
    """(FragmentOverlap over the scene's centroids, the oracle's keep mask on them)"""
    from lib.overlap import FragmentOverlap
    full = FragmentOverlap(D.scene_blob_case()[0], "FCGF", 0.025)
    xyz = full.xyz.cpu().numpy()
    res = D.dbscan(xyz, full.off, full.r, D.SCENE_SPEC["min_points"])
    assert D.margin(xyz, full.off, full.r) > 1e-9
    return full, D.cluster_keep(res, full.off, min_size=D.SCENE_SPEC["min_size"])


def test_register_scene_cluster_filter_removes_the_blobs(gpu):
    from lib.multiview import register_scene
    frags, blobs = D.scene_blob_case()
    init = O.scene4_starts(O.SIX, O.scene4_centroids())
    res = register_scene(frags, 0.025, init=init, method="point_to_plane", denoise=D.SCENE_SPEC)
    full, want_keep = _scene_oracle()
    assert set(res["denoise"]) == {"keep", "removed"} and res["denoise"]["keep"].dtype == bool
    np.testing.assert_array_equal(res["denoise"]["keep"], want_keep)
    removed = np.asarray([(~want_keep[full.off[b]:full.off[b + 1]]).sum() for b in range(full.B)])
    np.testing.assert_array_equal(res["denoise"]["removed"], removed)
    fo = full.select(want_keep)
    assert res["fo"].xyz.cpu().numpy().tobytes() == fo.xyz.cpu().numpy().tobytes()
    assert res["fo"].off.tolist() == fo.off.tolist()
    xyz = full.xyz.cpu().numpy()
    kept_by_radius = full.radius_outliers()["keep"].cpu().numpy()
    for b, blob in enumerate(blobs):
        rows = slice(full.off[b], full.off[b + 1])
        d = np.sqrt(((xyz[rows, None, :] - blob.astype(np.float64)[None]) ** 2).sum(2)).min(1)
        is_blob = d < 0.0434
        flying = np.sqrt(((xyz[rows, None, :] - K.scene_case()[1][b].astype(np.float64)[None]) ** 2).sum(2)).min(1) < 1e-6
        surface = ~is_blob & ~flying
        keep = res["denoise"]["keep"][rows]
        print("fragment %d: blob of %d centroids, the radius filter keeps %d of them, the cluster filter %d; %d of %d "
              "surface centroids removed" % (b, is_blob.sum(), kept_by_radius[rows][is_blob].sum(),
                                             keep[is_blob].sum(), (~keep[surface]).sum(), surface.sum()))
        assert is_blob.sum() >= 10 and kept_by_radius[rows][is_blob].mean() > 0.5
        assert not keep[is_blob].any() and (~keep[surface]).sum() <= 0.01 * surface.sum()
    # no fused point within half a voxel of a blob point's place in the scene
    fused = res["scene"]["xyz"].cpu().numpy()
    assert res["scene"]["n_points"].sum().item() == fo.M and len(fused) > 100
    for b, blob in enumerate(blobs):
        mapped = blob.astype(np.float64) @ res["R"][b].T + res["t"][b]
        assert np.sqrt(((fused[:, None, :] - mapped[None]) ** 2).sum(2)).min() > 0.0125, b


def test_register_scene_denoise_none_is_the_call_without_it(gpu):
    from lib.multiview import register_scene
    clean = O.scene4()[0]
    init = O.scene4_starts(O.SIX, O.scene4_centroids())
    a = register_scene(clean, 0.025, init=init, method="point_to_plane", denoise=None)
    b = register_scene(clean, 0.025, init=init, method="point_to_plane")
    assert set(a) == set(b) and "denoise" not in a
    assert a["poses"].tobytes() == b["poses"].tobytes() and a["pairs"]["T"].tobytes() == b["pairs"]["T"].tobytes()
    for k in ("xyz", "normals", "n_points", "n_frags"):
        assert a["scene"][k].cpu().numpy().tobytes() == b["scene"][k].cpu().numpy().tobytes(), k


def test_register_scene_cli_cluster_writes_what_register_scene_returns(gpu, tmp_path, capsys):
    from lib.multiview import register_scene
    from lib.ply import read_ply_xyz, write_ply_xyz
    from lib.utils import write_trajectory
    from scripts.fuse_scene import read_poses
    from scripts.register_scene import main, read_init
    frags = D.scene_blob_case()[0]
    files = []
    for b, f in enumerate(frags):
        files.append(str(tmp_path / ("frag_%d.ply" % b)))
        write_ply_xyz(files[-1], f)
    start = O.scene4_starts(O.SIX, O.scene4_centroids())
    write_trajectory(np.linalg.inv(start), [[i, j, True] for i, j in O.SIX], str(tmp_path / "init.txt"))
    out = str(tmp_path / "out")
    spec = D.SCENE_SPEC
    main(["--fragments"] + files + ["--out", out, "--init", str(tmp_path / "init.txt"), "--denoise",
                                    "cluster:%d:%d" % (spec["min_points"], spec["min_size"])])
    want = register_scene([read_ply_xyz(f) for f in files], 0.025, init=read_init(str(tmp_path / "init.txt"), 4),
                          denoise=spec)
    printed = capsys.readouterr().out
    assert "registered 4 fragments" in printed
    assert ("denoise (cluster): points removed per fragment: %s"
            % " ".join(str(int(v)) for v in want["denoise"]["removed"])) in printed
    assert (want["denoise"]["removed"] >= 10 + K.N_SCENE_PLANTED).all()
    np.testing.assert_allclose(read_poses(out + "/poses.txt", 4), want["poses"], rtol=0, atol=1e-11)
    blob = open(out + "/scene.ply", "rb").read()
    rows = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], "<f4").reshape(-1, 6)
    assert len(rows) > 100 and rows[:, :3].tobytes() == want["scene"]["xyz"].cpu().numpy().astype("<f4").tobytes()
