"""Multiview synchronisation of a scene's pairwise trajectory: traj.txt -> poses.txt + traj_sync.txt.

Reads the `traj.txt` the pairwise benchmark writes for a scene (scripts/benchmark_pairwise_registration.py: per
written pair the metadata `i j True` and, in the 3DMatch log convention, T_log = inv(T) of the estimate x_j ~ T x_i),
synchronises the pairs on the GPU (lib.multiview.synchronize) and writes into --out
  poses.txt      one block per fragment: metadata `i i N` and the 4 x 4 pose M_i (fragment i -> the anchor's frame),
  traj_sync.txt  the same pairs and flags with inv(M_j^-1 M_i): the synchronised pairwise estimates in the log
                 convention, readable by the benchmark's report code like any traj.txt.

With --info FILE --refine the synchronised poses are then refined jointly over SE(3) (lib.multiview.optimize_pose_graph)
with the information matrices of FILE (the est.info the benchmark's --write_info writes beside traj.txt: the same pairs
in the same order) and the IRLS weights the synchronisation returned; poses.txt and traj_sync.txt then hold the refined
poses, and the initial and final cost are printed.  Without the two flags nothing changes.  --line_process adds
Open3D's line process and edge pruning to the refinement (optimize_pose_graph(line_process=True): every pair is an
uncertain edge); --line_max_dist, the correspondence distance the information matrices were built with, is then
required, because est.info does not record it.

usage: python -m scripts.multiview_sync --traj results/RegBlock/all/<scene>/traj.txt --n_fragments 60 --out DIR
           [--anchor 0] [--irls 5] [--c_rot 0.1] [--c_trans 0.1] [--info est.info --refine [--refine_iters 20]
            [--line_process --line_max_dist D [--preference_loop_closure 1.0]]]
"""
import argparse
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from lib.utils import ensure_dir, read_trajectory, read_trajectory_info, write_trajectory  # noqa: E402
from lib.multiview import synchronize, pairwise_from_poses, optimize_pose_graph  # noqa: E402


def sync_trajectory(keys, traj, n_fragments, anchor=0, irls=0, c_rot=0.1, c_trans=0.1, info=None, refine_iters=20,
                    line_process=False, preference_loop_closure=1.0, line_max_dist=None):
    """keys [E,3] (i, j, flag) and traj [E,4,4] as read_trajectory returns them (T_log = inv(T)) ->
    (poses [N,4,4], traj_sync [E,4,4] in the log convention, the dict synchronize returned).
    info [E,6,6] (the pairs' information matrices, parameters (translation, rotation)): the synchronised poses are
    refined by optimize_pose_graph with them and the weights synchronize returned, for at most refine_iters trials;
    the returned dict then also holds `refined`, the dict optimize_pose_graph returned.  line_process: with the line
    process and edge pruning, every pair uncertain, line_max_dist the distance `info` was built with."""
    traj = np.asarray(traj, np.float64).reshape(-1, 4, 4)
    pairs = np.asarray([[int(k[0]), int(k[1])] for k in keys], np.int64).reshape(-1, 2)
    T = np.linalg.inv(traj) if len(traj) else traj
    res = synchronize(T[:, :3, :3], T[:, :3, 3], pairs, int(n_fragments), anchor=anchor, irls_iters=irls,
                      c_rot=c_rot, c_trans=c_trans)
    R, t = np.asarray(res["R"], np.float64), np.asarray(res["t"], np.float64)
    if info is not None:
        info = np.asarray(info, np.float64).reshape(-1, 6, 6)
        if len(info) != len(pairs):
            raise ValueError("the information file holds %d pairs, the trajectory %d" % (len(info), len(pairs)))
        ref = optimize_pose_graph(R, t, T[:, :3, :3], T[:, :3, 3], pairs, info, np.asarray(res["weights"]),
                                  anchor=anchor, max_iters=refine_iters,
                                  **({} if not line_process else dict(
                                      line_process=True, preference_loop_closure=preference_loop_closure,
                                      max_correspondence_distance=line_max_dist)))
        res = dict(res, refined=ref)
        R, t = np.asarray(ref["R"], np.float64), np.asarray(ref["t"], np.float64)
    poses = np.tile(np.eye(4), (int(n_fragments), 1, 1))
    poses[:, :3, :3], poses[:, :3, 3] = R, t
    T_sync = np.asarray(pairwise_from_poses(R, t, pairs), np.float64)
    return poses, (np.linalg.inv(T_sync) if len(T_sync) else T_sync), res


def write_poses(poses, filename):
    """one block per fragment in the trajectory files' layout: `i i N`, then the 4 rows of M_i"""
    n = poses.shape[0]
    with open(filename, "w") as f:
        for i in range(n):
            f.write("%d\t%d\t%d\n" % (i, i, n))
            f.write("\n".join("\t".join("{0:.12f}".format(v) for v in row) for row in poses[i].tolist()))
            f.write("\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--traj", required=True, help="a scene's traj.txt written by the pairwise benchmark")
    ap.add_argument("--n_fragments", type=int, required=True)
    ap.add_argument("--anchor", type=int, default=0)
    ap.add_argument("--irls", type=int, default=5, help="IRLS re-weighting passes (0: the plain closed form)")
    ap.add_argument("--c_rot", type=float, default=0.1)
    ap.add_argument("--c_trans", type=float, default=0.1)
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--info", default=None, help="the pairs' information matrices (est.info of the benchmark's "
                    "--write_info: the pairs of --traj in the same order)")
    ap.add_argument("--refine", action="store_true", help="refine the synchronised poses over SE(3) with --info")
    ap.add_argument("--refine_iters", type=int, default=20, help="--refine: the cap on Levenberg-Marquardt trials")
    ap.add_argument("--line_process", action="store_true", help="--refine with the line process and edge pruning of "
                    "Open3D's global_optimization (every pair an uncertain edge); needs --line_max_dist")
    ap.add_argument("--preference_loop_closure", type=float, default=1.0, help="--line_process: Open3D's option")
    ap.add_argument("--line_max_dist", type=float, default=None, help="--line_process: the correspondence distance "
                    "--info was built with (the benchmark's --info_max_dist)")
    a = ap.parse_args(argv)
    if a.refine != (a.info is not None):
        ap.error("--refine and --info go together")
    if a.line_process and not (a.refine and a.line_max_dist is not None):
        ap.error("--line_process needs --refine and --line_max_dist")
    keys, traj = read_trajectory(a.traj)
    info = read_trajectory_info(a.info)[1] if a.refine else None
    poses, traj_sync, res = sync_trajectory(keys, traj, a.n_fragments, a.anchor, a.irls, a.c_rot, a.c_trans,
                                            **({} if info is None else {"info": info, "refine_iters": a.refine_iters}),
                                            **({} if not a.line_process else dict(
                                                line_process=True, line_max_dist=a.line_max_dist,
                                                preference_loop_closure=a.preference_loop_closure)))
    ensure_dir(a.out)
    write_poses(poses, os.path.join(a.out, "poses.txt"))
    write_trajectory(traj_sync, [list(k) for k in keys], os.path.join(a.out, "traj_sync.txt"))
    member = np.asarray(res["member"])
    print("synchronised %d pairs over %d fragments (%d connected to anchor %d, status %d) -> %s"
          % (len(keys), a.n_fragments, int(member.sum()), a.anchor, int(np.asarray(res["status"])), a.out))
    if a.refine:
        ref = res["refined"]
        print("refined over SE(3): cost %.9g -> %.9g in %d trials (status %d)"
              % (float(ref["cost"][0]), float(ref["cost"][1]), int(ref["iters"]), int(ref["status"])))
        if a.line_process:
            print("line process: %d of %d pairs pruned, mu %.6g"
                  % (int((~np.asarray(ref["kept"])).sum()), len(keys), float(ref["mu"])))


if __name__ == "__main__":
    main()
