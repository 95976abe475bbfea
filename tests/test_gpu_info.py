"""GPU information matrices (csrc/info.hip mvr_pair_information, lib.icp.information_matrix) against the numpy
oracle (tests/info_oracle.py), which sums G^T G literally over the correspondences of icp_oracle.evaluate.

Bounds: n_corr and status exactly; rmse to 1e-12 relative; |info_gpu - info_oracle|_F <= 1e-11 |info_oracle|_F (fp64
summation of at most about 2e4 terms: gamma_n ~ 4e-12 times the sum of magnitudes, which the diagonal dominates).
Every case first asserts the oracle's margins (gap, edge >= 1e-8), so that no correspondence is decided by rounding."""
import functools

import numpy as np
import pytest

import icp_oracle as O
import info_oracle as IO

pytestmark = pytest.mark.gpu
TOL_INFO, TOL_RMSE, MARGIN = 1e-11, 1e-12, 1e-8


@functools.lru_cache(maxsize=None)
def _fo(name):
    from lib.overlap import FragmentOverlap
    if name.startswith("centroids"):
        return FragmentOverlap(O.scene4()[0], "FCGF", 0.025)
    case = [c for c in IO.cases() if c[0] == name][0]
    return FragmentOverlap(list(case[1]), "3DMatch", radius={"pair": 0.06, "small": O.SMALL_RADIUS,
                                                             "full_copy": 0.05}[name])


def _points(fo):
    """the fragments as the index holds them (for 'FCGF' the centroids in the GPU's row order)"""
    xyz = fo.xyz.cpu().numpy()
    return [xyz[fo.off[b]:fo.off[b + 1]] for b in range(fo.B)]


def _compare(name, got, want, max_dist):
    assert min(w["gap"] for w in want) >= MARGIN and min(w["edge"] for w in want) >= MARGIN, name
    for k, w in enumerate(want):
        assert int(got["n_corr"][k]) == w["n_corr"] and int(got["status"][k]) == w["status"], (name, k)
        L = got["info"][k]
        fro = np.linalg.norm(w["info"])
        d = np.linalg.norm(L - w["info"])
        dr = abs(got["rmse"][k] - w["rmse"])
        print("%s pair %d: n_corr %d, |d info|_F / |info|_F %.3g, |d rmse| / rmse %.3g"
              % (name, k, w["n_corr"], d / fro if fro else d, dr / w["rmse"] if w["rmse"] else dr))
        assert d <= TOL_INFO * fro, (name, k)
        # an exact copy at its true motion leaves an rmse of rounding noise (1e-16): nothing relative to compare
        assert dr <= TOL_RMSE * (w["rmse"] if w["rmse"] > 1e-9 * max_dist else max_dist), (name, k)
        assert L[0, 0] == L[1, 1] == L[2, 2] == w["n_corr"]
        np.testing.assert_array_equal(L, L.T)
        np.testing.assert_array_equal(L[:3, :3], w["n_corr"] * np.eye(3))


@pytest.mark.parametrize("name", ["centroids", "centroids_0.03", "pair", "small", "full_copy"])
def test_matches_oracle(gpu, name):
    from lib.icp import icp_refine, information_matrix
    _, _, pairs, T, max_dist = [c for c in IO.cases() if c[0] == name][0]
    fo = _fo(name)
    got = information_matrix(fo, pairs, T, max_dist)
    want = IO.information_batch(_points(fo), pairs, T, max_dist)
    _compare(name, got, want, max_dist)
    assert got["info"].shape == (len(pairs), 6, 6) and got["info"].dtype == np.float64
    ev = icp_refine(fo, pairs, T, max_dist, max_iters=0)                    # the same eval(T)
    np.testing.assert_array_equal(got["n_corr"], ev["n_corr"])
    if name == "centroids":                                                 # and the overlap gate's counts at fo.r
        c_ij = fo.counts(O.SIX, np.linalg.inv(T[:6]))[:, 0]
        c_ji = fo.counts(O.SIX, T[6:])[:, 1]
        np.testing.assert_array_equal(got["n_corr"], np.concatenate([c_ij, c_ji]))
        assert got["n_corr"].min() > 500
    if name == "small":
        sizes = [len(_points(fo)[s]) for s, _ in pairs]
        assert sorted(sizes[:8] + sizes[9:11]) == list(IO.SIZES) and sizes[8] == 40 and sizes[11] == 3
        assert got["n_corr"][:4].tolist() == [0, 1, 2, 3] and got["n_corr"][8] == 0 and got["n_corr"][11] == 0
        assert not got["info"][[0, 8, 11]].any() and (got["status"] == 0).all()
    if name == "full_copy":
        assert got["n_corr"][1] == len(_points(fo)[0]) and got["rmse"][1] < 1e-12


def _raw_call(fo, pairs, T, max_dist, sentinel=-77.0):
    """mvr_pair_information on sentinel-filled output buffers -> numpy outputs"""
    import torch
    from lib import _native as N
    d = fo.device
    P = len(pairs)
    gp = torch.as_tensor(np.asarray(pairs, np.int64)).to(d)
    gT = torch.as_tensor(np.ascontiguousarray(np.asarray(T, np.float64)[:, :3])).to(d)
    info = torch.full((P, 36), sentinel, dtype=torch.float64, device=d)
    rm = torch.full((P,), sentinel, dtype=torch.float64, device=d)
    nc, st = (torch.full((P,), int(sentinel), dtype=torch.int32, device=d) for _ in range(2))
    rc = N.lib().mvr_pair_information(N.ptr(fo.index), fo.index.numel(), N.ptr(fo.xyz), N.ptr(fo.off_dev), fo.B, fo.M,
                                      fo.r, N.ptr(gp), N.ptr(gT), P, max_dist, N.ptr(info), N.ptr(nc), N.ptr(rm),
                                      N.ptr(st), N.stream())
    return rc, {"info": info.cpu().numpy().reshape(P, 6, 6), "rmse": rm.cpu().numpy(), "n_corr": nc.cpu().numpy(),
                "status": st.cpu().numpy()}


def test_invalid_pairs_and_their_neighbours(gpu):
    frags, pairs, T = IO.small_case_all_sizes()
    fo = _fo("small")
    T = T.copy()
    pairs = pairs.copy()
    bad = {2: "nan", 5: "index -1", 6: "index B", 9: "inf"}
    T[2, 1, 2] = np.nan
    pairs[5, 0] = -1
    pairs[6, 1] = fo.B
    T[9, 0, 3] = np.inf
    rc, got = _raw_call(fo, pairs, T, O.SMALL_MAX_DIST)
    assert rc == 0
    for name in got:
        assert not np.any(got[name] == -77.0), name                         # every row of every output is written
    want = IO.information_batch(_points(fo), pairs, T, O.SMALL_MAX_DIST)
    assert [w["status"] for w in want] == [4 if k in bad else 0 for k in range(len(pairs))]
    _compare("small+invalid", got, want, O.SMALL_MAX_DIST)
    for k in bad:
        assert not got["info"][k].any() and (got["n_corr"][k], got["rmse"][k], got["status"][k]) == (0, 0.0, 4)
    ok = [k for k in range(len(pairs)) if k not in bad]                      # the neighbours: as without them
    rc, alone = _raw_call(fo, pairs[ok], T[ok], O.SMALL_MAX_DIST)
    for name in alone:
        assert alone[name].tobytes() == got[name][ok].tobytes(), name


def test_outputs_do_not_depend_on_the_batch(gpu):
    from lib.icp import information_matrix
    fo = _fo("centroids")
    T12 = O.eval_starts(O.scene4_centroids())
    rows = np.arange(70) % 12
    pairs, T = np.asarray(O.TWELVE)[rows], T12[rows]
    for k in (3, 8):                                                        # a ground-truth and a perturbed row
        one = information_matrix(fo, pairs[k:k + 1], T[k:k + 1])
        assert one["n_corr"][0] > 500
        for pos in (0, 34, 69):                                             # first, in the middle, last of 70
            p, t = pairs.copy(), T.copy()
            p[pos], t[pos] = pairs[k], T[k]
            got = information_matrix(fo, p, t)
            for name in one:
                assert got[name][pos].tobytes() == one[name][0].tobytes(), (k, pos, name)


def test_max_dist_rules_and_python_surface(gpu):
    import torch
    from lib.icp import information_matrix
    fo = _fo("centroids")
    T = O.eval_starts(O.scene4_centroids())
    ref = information_matrix(fo, O.TWELVE, T, max_dist=fo.r)               # max_dist == r_index: accepted
    dflt = information_matrix(fo, O.TWELVE, T)
    for name in ref:
        assert isinstance(ref[name], np.ndarray) and ref[name].tobytes() == dflt[name].tobytes(), name
    with pytest.raises(ValueError, match="exceeds"):
        information_matrix(fo, O.TWELVE, T, max_dist=fo.r * (1 + 1e-12))
    rc, _ = _raw_call(fo, O.TWELVE, T, fo.r * (1 + 1e-12))
    assert rc == -1
    rc, raw = _raw_call(fo, O.TWELVE, T, fo.r)
    assert rc == 0 and raw["info"].tobytes() == ref["info"].tobytes()
    # the Open3D order: the blocks swapped
    o3d = information_matrix(fo, O.TWELVE, T, order="open3d")
    np.testing.assert_array_equal(o3d["info"], IO.to_open3d(ref["info"]))
    np.testing.assert_array_equal(o3d["info"][:, 3, 3], ref["n_corr"])
    # torch on the device in -> torch on the device out, the same bits; [P,3,4] fp32 on the host -> torch on the host
    dev = information_matrix(fo, torch.tensor(O.TWELVE, device=gpu), torch.from_numpy(T).to(gpu))
    assert all(torch.is_tensor(v) and v.device.type == "cuda" for v in dev.values())
    assert dev["info"].shape == (12, 6, 6) and dev["n_corr"].dtype == torch.int32
    for name in ref:
        assert dev[name].cpu().numpy().tobytes() == ref[name].tobytes(), name
    T32 = torch.from_numpy(T[:, :3].astype(np.float32))
    host = information_matrix(fo, O.TWELVE, T32)
    want = information_matrix(fo, O.TWELVE, T32.numpy().astype(np.float64))
    assert all(torch.is_tensor(v) and v.device.type == "cpu" for v in host.values())
    for name in want:
        assert host[name].numpy().tobytes() == want[name].tobytes(), name
    empty = information_matrix(fo, np.zeros((0, 2), np.int64), np.zeros((0, 4, 4)))
    assert empty["info"].shape == (0, 6, 6) and empty["n_corr"].shape == (0,)
