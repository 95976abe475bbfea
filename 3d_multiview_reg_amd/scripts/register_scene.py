"""Fragments in, registered scene out, without a pretrained network: PLY files -> poses.txt, traj.txt, scene.ply.

lib.multiview.register_scene on the fragments' PLY files: voxel centroids, normals, FPFH + RANSAC on all pairs
(or the pairwise estimates of --init), the overlap gate, ICP, information matrices, synchronisation, pose-graph
refinement and the fused cloud, all on the GPU.  Writes into --out
  poses.txt   one block per fragment: `i i N` and the 4 x 4 pose M_i (fragment i -> the anchor's frame),
  traj.txt    the pairs that passed the overlap gate, `i j True` and inv(T) of the refined estimate x_j ~ T x_i (the
              3DMatch log convention of the pairwise benchmark's traj.txt, readable by scripts/multiview_sync.py),
  scene.ply   the fused cloud with normals (scripts/fuse_scene.py fuses again at another voxel size from poses.txt).
--init traj.txt: a trajectory in that convention holding every pair i < j replaces the FPFH stage.
--line_process: the pose-graph refinement runs with Open3D's line process and edge pruning (every pair that passed the
gate is an uncertain edge); the pairs it pruned are counted in the printed line.
--denoise statistical:20:2.0 | radius:16[:R]: Open3D's statistical / radius outlier removal on each fragment's centroids
before anything else uses them; the points removed per fragment are printed.
--denoise cluster:MIN_POINTS:MIN_SIZE[:EPS]: Open3D's cluster_dbscan(EPS, MIN_POINTS) on each fragment's centroids (EPS
defaults to 3 voxel sizes, its largest value); the clusters of fewer than MIN_SIZE points and the noise are removed.
--keypoints iss[:SALIENT:NONMAX]: ISS keypoints (Open3D's compute_iss_keypoints; radii default to 3 and 2 voxel sizes)
are detected on each fragment and the FPFH matching runs on them alone; the keypoints per fragment are printed.
--icp_kernel huber|cauchy|gm|tukey|l2[:K]: the ICP stage weighs every correspondence by a robust kernel of scale K
(K defaults to the voxel size; lib.icp.ROBUST_KERNELS); the kernel and its scale are printed.
--icp_method colored: coloured ICP (Open3D's registration_colored_icp) on the red / green / blue properties of the
fragments' PLY files, which must all have them; --icp_lambda_geometric is the share of the geometric term.

usage: python -m scripts.register_scene --fragments F0.ply F1.ply ... --out DIR [--voxel_size 0.025]
           [--icp_method point_to_point | colored [--icp_lambda_geometric 0.968]] [--init traj.txt] [--dataset 3d_match] [--min_frags 1] [--seed 0]
           [--checkers | --coarse fgr] [--line_process [--preference_loop_closure 1.0]] [--denoise statistical:20:2.0]
           [--keypoints iss[:SALIENT:NONMAX]] [--icp_kernel tukey[:K]]
"""
import argparse
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from lib.ply import read_ply_colors, read_ply_xyz, write_ply  # noqa: E402
from lib.utils import ensure_dir, read_trajectory, write_trajectory  # noqa: E402
from scripts.multiview_sync import write_poses  # noqa: E402

ICP_METHODS = ("point_to_point", "point_to_plane", "generalized", "colored")   # lib.multiview.ICP_METHODS
DATASETS = ("3d_match", "redwood")                                  # lib.multiview.OVERLAP_THRESHOLDS
COARSE_METHODS = ("ransac", "fgr")                                  # lib.multiview.COARSE_METHODS
ROBUST_KERNELS = ("l2", "huber", "cauchy", "gm", "tukey")           # lib.icp.ROBUST_KERNELS


def read_init(filename, n_fragments):
    """a traj.txt (T_log = inv(T)) holding every pair i < j -> [P,4,4] estimates x_j ~ T x_i in the order of the
    pairs i < j"""
    keys, traj = read_trajectory(filename)
    by_pair = {(int(k[0]), int(k[1])): np.linalg.inv(T) for k, T in zip(keys, traj)}
    want = [(i, j) for i in range(n_fragments) for j in range(i + 1, n_fragments)]
    missing = [p for p in want if p not in by_pair]
    if missing:
        raise ValueError("%s: no estimate for the pairs %s" % (filename, missing[:8]))
    return np.asarray([by_pair[p] for p in want], dtype=np.float64).reshape(-1, 4, 4)


def parse_denoise(text):
    """'statistical:NB:RATIO', 'radius:NB[:R]' or 'cluster:MIN_POINTS:MIN_SIZE[:EPS]' -> register_scene's denoise dict
    (ValueError on anything else)"""
    parts = text.split(":")
    try:
        if parts[0] == "statistical" and len(parts) == 3:
            d = {"method": "statistical", "nb_neighbors": int(parts[1]), "std_ratio": float(parts[2])}
        elif parts[0] == "radius" and len(parts) in (2, 3):
            d = {"method": "radius", "nb_points": int(parts[1]), "radius": float(parts[2]) if len(parts) == 3 else None}
        elif parts[0] == "cluster" and len(parts) in (3, 4):
            d = {"method": "cluster", "min_points": int(parts[1]), "min_size": int(parts[2]),
                 "eps": float(parts[3]) if len(parts) == 4 else None}
        else:
            raise ValueError("neither form")
    except ValueError:
        raise ValueError("--denoise must be statistical:NB_NEIGHBORS:STD_RATIO, radius:NB_POINTS[:RADIUS] or "
                         "cluster:MIN_POINTS:MIN_SIZE[:EPS], not %r" % (text,))
    return d


def parse_keypoints(text):
    """'iss' or 'iss:SALIENT:NONMAX' -> register_scene's keypoints dict (ValueError on anything else)"""
    parts = text.split(":")
    try:
        if parts[0] == "iss" and len(parts) == 1:
            d = {}
        elif parts[0] == "iss" and len(parts) == 3:
            d = {"salient_radius": float(parts[1]), "non_max_radius": float(parts[2])}
        else:
            raise ValueError("neither form")
    except ValueError:
        raise ValueError("--keypoints must be iss or iss:SALIENT_RADIUS:NON_MAX_RADIUS, not %r" % (text,))
    return d


def parse_icp_kernel(text):
    """'NAME' or 'NAME:K' -> (name, K or None) of register_scene's icp_kernel / icp_kernel_k (ValueError on anything
    else)"""
    parts = text.split(":")
    try:
        if parts[0] not in ROBUST_KERNELS or len(parts) > 2:
            raise ValueError("neither form")
        k = float(parts[1]) if len(parts) == 2 else None
        if k is not None and not k > 0.0:
            raise ValueError("K not positive")
    except ValueError:
        raise ValueError("--icp_kernel must be NAME or NAME:K with NAME one of %s and K > 0, not %r"
                         % (", ".join(ROBUST_KERNELS), text))
    return parts[0], k


def read_colored_fragments(paths):
    """the fragments' points and colours for --icp_method colored (ValueError naming the files without red / green /
    blue) -> (xyz list, colors list)"""
    both = [read_ply_colors(f) for f in paths]
    bare = [f for f, (_, c) in zip(paths, both) if c is None]
    if bare:
        raise ValueError("--icp_method colored needs red, green and blue vertex properties; none in %s"
                         % ", ".join(bare))
    return [x for x, _ in both], [c for _, c in both]


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fragments", required=True, nargs="+", help="the fragments' PLY files (at least two)")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--voxel_size", type=float, default=0.025, help="voxel size of the centroids and of the scene")
    ap.add_argument("--icp_method", default="point_to_point", choices=ICP_METHODS)
    ap.add_argument("--icp_lambda_geometric", type=float, default=0.968,
                    help="--icp_method colored: the share of the geometric term, in [0, 1] (Open3D's lambda_geometric)")
    ap.add_argument("--init", default=None, help="traj.txt with an estimate for every pair i < j instead of FPFH")
    ap.add_argument("--dataset", default="3d_match", choices=DATASETS,
                    help="the overlap gate's threshold, as the pairwise benchmark picks it: 0.3 / 0.23")
    ap.add_argument("--min_frags", type=int, default=1, help="keep the voxels at least so many fragments fell into")
    ap.add_argument("--anchor", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0, help="RANSAC draw stream seed")
    ap.add_argument("--checkers", action="store_true",
                    help="RANSAC with the edge-length and distance checkers: 3-point samples, 100000 draws")
    ap.add_argument("--coarse", default="ransac", choices=COARSE_METHODS,
                    help="the coarse estimate from the FPFH matches: RANSAC, or Fast Global Registration (for matches "
                         "with tens of percent inliers; not with --checkers)")
    ap.add_argument("--line_process", action="store_true",
                    help="pose-graph refinement with the line process and edge pruning of Open3D's global_optimization")
    ap.add_argument("--preference_loop_closure", type=float, default=1.0, help="--line_process: Open3D's option")
    ap.add_argument("--denoise", default=None, metavar="SPEC",
                    help="remove outliers from the centroids before registration: statistical:20:2.0 (Open3D's "
                         "remove_statistical_outlier(nb_neighbors, std_ratio)) or radius:16[:R] "
                         "(remove_radius_outlier(nb_points, radius), R at most 3 voxel_size, its default), or keep "
                         "the DBSCAN clusters of at least MIN_SIZE points: cluster:10:100[:EPS] "
                         "(cluster_dbscan(eps, min_points), EPS at most 3 voxel_size, its default)")
    ap.add_argument("--keypoints", default=None, metavar="SPEC",
                    help="match the FPFH descriptors of ISS keypoints only: iss, or iss:SALIENT:NONMAX (Open3D's "
                         "compute_iss_keypoints radii, each at most 3 voxel_size; defaults 3 and 2 voxel_size); not "
                         "with --init")
    ap.add_argument("--icp_kernel", default=None, metavar="NAME[:K]",
                    help="weigh the ICP correspondences by a robust kernel: huber, cauchy, gm, tukey or l2, with its "
                         "scale K (Open3D's RobustKernel; K defaults to the voxel size, for gm a squared length)")
    return ap


def check_args(ap, a):
    if len(a.fragments) < 2:
        ap.error("--fragments needs at least two files")
    if not a.voxel_size > 0.0:
        ap.error("--voxel_size must be positive")
    if a.min_frags < 1:
        ap.error("--min_frags must be at least 1")
    if not 0 <= a.anchor < len(a.fragments):
        ap.error("--anchor outside the fragments")
    if a.coarse == "fgr" and a.checkers:
        ap.error("--checkers belongs to --coarse ransac")
    if not 0.0 <= a.icp_lambda_geometric <= 1.0:
        ap.error("--icp_lambda_geometric must lie in [0, 1]")
    if not a.preference_loop_closure > 0.0:
        ap.error("--preference_loop_closure must be positive")
    if a.denoise is not None:
        from lib.multiview import _denoise_arguments
        try:
            a.denoise = _denoise_arguments(parse_denoise(a.denoise), 3.0 * a.voxel_size)
        except ValueError as e:
            ap.error(str(e))
    if a.keypoints is not None:
        from lib.multiview import _keypoints_arguments
        try:
            a.keypoints = _keypoints_arguments(parse_keypoints(a.keypoints), 3.0 * a.voxel_size, a.init)
        except ValueError as e:
            ap.error(str(e))
    if a.icp_kernel is not None:
        try:
            a.icp_kernel = parse_icp_kernel(a.icp_kernel)
        except ValueError as e:
            ap.error(str(e))
    return a


def main(argv=None):
    from lib.multiview import register_scene
    ap = parser()
    a = check_args(ap, ap.parse_args(argv))
    colors = None
    if a.icp_method == "colored":
        frags, colors = read_colored_fragments(a.fragments)
    else:
        frags = [read_ply_xyz(f) for f in a.fragments]
    init = None if a.init is None else read_init(a.init, len(frags))
    res = register_scene(frags, a.voxel_size, method=a.icp_method, init=init, dataset=a.dataset, seed=a.seed,
                         anchor=a.anchor, min_frags=a.min_frags, ransac_checkers=a.checkers,
                         **({} if colors is None else dict(colors=colors,
                                                           icp_lambda_geometric=a.icp_lambda_geometric)),
                         **({} if a.coarse == "ransac" else dict(coarse=a.coarse)),
                         **({} if not a.line_process else dict(line_process=True,
                                                               preference_loop_closure=a.preference_loop_closure)),
                         **({} if a.denoise is None else dict(denoise=a.denoise)),
                         **({} if a.keypoints is None else dict(keypoints=a.keypoints)),
                         **({} if a.icp_kernel is None else dict(icp_kernel=a.icp_kernel[0],
                                                                 icp_kernel_k=a.icp_kernel[1])))
    ensure_dir(a.out)
    write_poses(res["poses"], os.path.join(a.out, "poses.txt"))
    rec = res["pairs"]
    meta = [[int(i), int(j), bool(k)] for (i, j), k in zip(rec["pairs"], rec["kept"])]
    write_trajectory(np.linalg.inv(rec["T"]), meta, os.path.join(a.out, "traj.txt"))
    scene = res["scene"]
    write_ply(os.path.join(a.out, "scene.ply"), scene["xyz"].cpu().numpy(),
              None if scene["normals"] is None else scene["normals"].cpu().numpy())
    print("registered %d fragments: %d of %d pairs passed the overlap gate, %d fragments connected to anchor %d; "
          "pose-graph cost %.6g -> %.6g; %d voxels of %g -> %s"
          % (len(frags), int(rec["kept"].sum()), len(meta), int(np.asarray(res["member"]).sum()), a.anchor,
             float(res["refined"]["cost"][0]), float(res["refined"]["cost"][1]), len(scene["xyz"]), a.voxel_size,
             a.out))
    if a.denoise is not None:
        print("denoise (%s): points removed per fragment: %s"
              % (a.denoise["method"], " ".join(str(int(v)) for v in res["denoise"]["removed"])))
    if a.keypoints is not None:
        print("keypoints (iss): per fragment: %s" % " ".join(str(int(v)) for v in np.diff(res["keypoints"]["off"])))
    if a.icp_kernel is not None:
        print("icp kernel: %s, k %g" % (a.icp_kernel[0], a.voxel_size if a.icp_kernel[1] is None else a.icp_kernel[1]))
    if a.line_process:
        print("line process: %d of the %d gated pairs pruned" % (int(rec["pruned"].sum()), int(rec["kept"].sum())))
    return res


if __name__ == "__main__":
    main()
