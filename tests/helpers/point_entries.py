"""The per-point entries on the radius index (csrc/rindex.hpp) through the C ABI on outputs allocated
full of a sentinel: what tests/test_gpu_gicp.py::test_per_point_entries_share_one_walk and the case set `points` of
tools/lib_ab.py both run."""
import numpy as np

SENT = -77          # what an entry does not write stays: fp64 / fp32 -77.0, int32 -77, uint8 179
ISS = {"gamma_21": 0.975, "gamma_32": 0.975, "min_ratio": 1e-6, "min_neighbors": 5}
STAT_K, STAT_RATIO = 20, 2.0


def run(d, L, frags, r_index, radius, ks=(1, 20, 64)):
    """mvr_radius_index_build on `frags` at cell r_index, then over balls of `radius`: mvr_estimate_normals without
    and with viewpoints, mvr_iss_saliency, mvr_radius_nms on that saliency, mvr_radius_count, mvr_color_gradient on
    seeded colours and the normals just computed (the unoriented ones), mvr_compute_fpfh on them with spfh_out,
    mvr_knn_self at every k of ks and mvr_statistical_outlier on the distances at STAT_K (if in ks).
    -> {"entry output": device tensor}, every entry's outputs whole"""
    import torch
    from lib import _native as N

    def full(dtype, *shape):
        return torch.full(shape, SENT & 0xff if dtype == torch.uint8 else SENT, dtype=dtype, device=d)
    f64, f32, i32, u8 = torch.float64, torch.float32, torch.int32, torch.uint8
    B = len(frags)
    off = np.concatenate([[0], np.cumsum([len(f) for f in frags])]).astype(np.int64)
    M = int(off[-1])
    xyz = torch.from_numpy(np.concatenate([np.asarray(f, np.float64).reshape(-1, 3) for f in frags])).to(d)
    g_off = torch.from_numpy(off).to(d)
    ib = L.mvr_radius_index_bytes(M)
    index = torch.empty(ib, dtype=u8, device=d)
    N.check(L.mvr_radius_index_build(N.ptr(xyz), N.ptr(g_off), B, M, r_index, N.ptr(index), ib, N.stream()),
            "mvr_radius_index_build")
    head, tail = (N.ptr(index), ib, N.ptr(xyz)), (N.ptr(g_off), B, M, r_index)
    vp = torch.from_numpy(np.array([[0.1 * b, -0.05 * b, 1.0] for b in range(B)])).to(d)
    colors = torch.from_numpy(np.random.default_rng(11).uniform(0.0, 1.0, (M, 3))).to(d)
    o = {}
    for tag, v in (("normals", None), ("normals vp", vp)):
        o[tag + " normals"], o[tag + " n_nbr"] = full(f64, M, 3), full(i32, M)
        N.check(L.mvr_estimate_normals(*head, *tail, radius, N.ptr(v), N.ptr(o[tag + " normals"]),
                                       N.ptr(o[tag + " n_nbr"]), N.stream()), "mvr_estimate_normals")
    o["iss saliency"], o["iss n_nbr"], o["nms keep"] = full(f64, M), full(i32, M), full(u8, M)
    N.check(L.mvr_iss_saliency(*head, *tail, radius, ISS["gamma_21"], ISS["gamma_32"], ISS["min_ratio"],
                               ISS["min_neighbors"], N.ptr(o["iss saliency"]), N.ptr(o["iss n_nbr"]), N.stream()),
            "mvr_iss_saliency")
    N.check(L.mvr_radius_nms(*head, *tail, radius, ISS["min_neighbors"], N.ptr(o["iss saliency"]),
                             N.ptr(o["nms keep"]), N.stream()), "mvr_radius_nms")
    o["count count"] = full(i32, M)
    N.check(L.mvr_radius_count(*head, *tail, radius, N.ptr(o["count count"]), N.stream()), "mvr_radius_count")
    nrm = o["normals normals"]
    o["color intensity"], o["color grad"], o["color n_nbr"] = full(f64, M), full(f64, M, 3), full(i32, M)
    N.check(L.mvr_color_gradient(*head, N.ptr(nrm), N.ptr(colors), *tail, radius, N.ptr(o["color intensity"]),
                                 N.ptr(o["color grad"]), N.ptr(o["color n_nbr"]), N.stream()), "mvr_color_gradient")
    o["fpfh fpfh"], o["fpfh spfh"] = full(f32, M, 33), full(f32, M, 33)
    ws = torch.empty(L.mvr_compute_fpfh_workspace_bytes(M), dtype=u8, device=d)
    N.check(L.mvr_compute_fpfh(*head, N.ptr(nrm), *tail, radius, N.ptr(o["fpfh fpfh"]), N.ptr(o["fpfh spfh"]),
                               N.ptr(ws), ws.numel(), N.stream()), "mvr_compute_fpfh")
    ws = torch.empty(L.mvr_knn_self_workspace_bytes(M), dtype=u8, device=d)
    for k in ks:
        idx, dist2 = full(i32, M, k), full(f64, M, k)
        N.check(L.mvr_knn_self(*head, *tail, k, N.ptr(idx), N.ptr(dist2), N.ptr(ws), ws.numel(), N.stream()),
                "mvr_knn_self")
        o["knn%d idx" % k], o["knn%d dist2" % k] = idx, dist2
        if k == STAT_K:
            o["stat keep"], o["stat mean_dist"], o["stat thr"] = full(u8, M), full(f64, M), full(f64, B)
            N.check(L.mvr_statistical_outlier(N.ptr(dist2), N.ptr(g_off), B, M, k, STAT_RATIO, N.ptr(o["stat keep"]),
                                              N.ptr(o["stat mean_dist"]), N.ptr(o["stat thr"]), N.stream()),
                    "mvr_statistical_outlier")
    torch.cuda.synchronize()
    return o
