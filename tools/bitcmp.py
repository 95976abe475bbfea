"""Bit-identity check between two builds of libmvreg_hip.so (tools' A/B variants, MVR_LIB).
  python tools/bitcmp.py dump <out.npz>      run the strict train-mode OANet fixture (32 pairs x 5000, both blocks:
                                             logits, scores, R, t), one scene step of the bench workload (records
                                             of all 435 pairs) and the radius-index refinements (the three ICP
                                             methods and mvr_pair_information on the tests' scene and small shapes:
                                             every output) and the pose-graph refinement (mvr_posegraph_optimize
                                             on seeded scenes of tests/posegraph_oracle.py: every output), save
                                             them; `dump <out.npz> posegraph` (or oanet, scene, refinements): only
                                             those sections
  python tools/bitcmp.py cmp <a.npz> <b.npz> count the elements that differ bit for bit (exit 1 if any)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d_multiview_reg_amd"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)


def refinements():
    """every output of icp_refine (both methods), gicp_refine and information_matrix: the 4-fragment scene's six pairs
    over 30 iterations at tolerances 0, and the tests' small shapes"""
    import icp_oracle as O
    import icp_plane_oracle as PO
    import info_oracle as IO
    from lib.icp import gicp_refine, icp_refine, information_matrix
    from lib.overlap import FragmentOverlap
    kw = dict(max_iters=30, tol_fitness=0.0, tol_rmse=0.0, return_trace=True)
    runs = {"p2p": lambda *a: icp_refine(*a, **kw), "p2l": lambda *a: icp_refine(*a, method="point_to_plane", **kw),
            "gicp": lambda *a: gicp_refine(*a, **kw), "info": information_matrix}
    res = {}

    def add(case, fo, pairs, T0, max_dist, which):
        for name in which:
            for k, v in runs[name](fo, pairs, T0, max_dist).items():
                res["%s_%s_%s" % (case, name, k)] = v

    fo = FragmentOverlap(O.scene4()[0], "FCGF", 0.025)
    fo.estimate_normals()
    add("six", fo, O.SIX, O.scene4_starts(O.SIX, O.scene4_centroids()), 0.075, runs)
    frags, pairs, T0 = O.small_case()
    add("small", FragmentOverlap(frags, "3DMatch", radius=O.SMALL_RADIUS), pairs, T0, O.SMALL_MAX_DIST, ["p2p"])
    fo = FragmentOverlap(PO.small_normals_case(), "3DMatch", radius=PO.SMALL_R_INDEX)
    fo.estimate_normals()
    add("smalln", fo, *PO.small_normals_pairs(), PO.SMALL_R_INDEX, runs)
    _, frags, pairs, T, max_dist = [c for c in IO.cases() if c[0] == "small"][0]
    add("smallinfo", FragmentOverlap(list(frags), "3DMatch", radius=O.SMALL_RADIUS), pairs, T, max_dist, ["info"])
    return res


def posegraph():
    """every output of optimize_pose_graph (the plain entry, mvr_posegraph_optimize) on seeded scenes of
    tests/posegraph_oracle.py, alone and as one ragged batch"""
    import posegraph_oracle as PO
    from lib.multiview import optimize_pose_graph
    keys = ("R0", "t0", "R_pair", "t_pair", "ij", "info", "w")
    C = PO.cases()
    res = {}
    runs = [("n30_noisy", dict(max_iters=6, tol_cost=0.0, tol_step=0.0)), ("n30_noisy", {})]
    runs += [(n, C[n][1]) for n in ("n30_noisy_tol", "n64_noisy", "reject", "bad_edges", "edges_257", "n30_exact")]
    for name, kw in runs:
        tag = "pg_%s%s" % (name, "" if kw else "_default")
        for k, v in optimize_pose_graph(*(C[name][0][k] for k in keys), return_trace=True, **kw).items():
            res["%s_%s" % (tag, k)] = np.asarray(v)
    scs = [C[n][0] for n in ("n3_noisy", "n30_noisy", "bad_edges", "disconnected")]
    out = optimize_pose_graph(*([s[k] for s in scs] for k in keys), return_trace=True, max_iters=3, tol_cost=0.0,
                              tol_step=0.0)
    for k, v in out.items():
        res["pg_batch_%s" % k] = np.asarray(v)
    return res


SECTIONS = ("oanet", "scene", "refinements", "posegraph")


def dump(path, sections=SECTIONS):
    res = {}
    if "posegraph" in sections:
        res.update(posegraph())
    if "refinements" in sections:
        res.update(refinements())
    if "oanet" in sections or "scene" in sections:
        res.update(network(sections))
    np.savez(path, **res)
    print("dumped", path, {k: v.shape for k, v in res.items()})


def network(sections):
    import json
    import torch
    import bench
    from synth import synth_correspondences
    dev = torch.device("cuda", 0)
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "oanet_full_train_strict.npz")))
    p = json.loads(str(g["params"]))
    xs, _, _ = synth_correspondences(32, 5000, seed=p["xs_seed"], inlier_lo=p["inlier_lo"], inlier_hi=p["inlier_hi"])
    out, _ = bench._oanet_golden(dev, "oanet_full_train_strict.npz", p["weights_seed"], xs)
    res = {}
    if "oanet" in sections:
        for i in range(2):
            for k in ("logits", "scores", "rot_est", "trans_est"):
                res["%s%d" % (k, i)] = out[k][i].detach().cpu().numpy()
    if "scene" in sections:
        wl = bench.SceneWorkload(dev, 0)
        with torch.no_grad():
            res["scene_records"] = wl.step().cpu().numpy()
    return res


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    bad = 0
    for k in A.files:
        x, y = A[k], B[k]
        n = int((x.view(np.uint32) != y.view(np.uint32)).sum()) if x.dtype == np.float32 else int((x != y).sum())
        bad += n
        print("%-16s %8d of %9d differ, max |diff| %.3g" % (k, n, x.size, float(np.abs(x - y).max()) if x.size else 0.0))
    print("BIT-IDENTICAL" if bad == 0 else "DIFFERENT")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], tuple(sys.argv[3:]) or SECTIONS)
    else:
        sys.exit(1 if cmp(sys.argv[2], sys.argv[3]) else 0)
