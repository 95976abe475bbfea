"""Pairwise registration demo (scripts/pairwise_demo.py of the reference): two point clouds -> the relative
transformation, written to ./data/demo/pairwise/results/est_T.log.

Same CLI and output file as the reference; the whole chain runs on the GPU through the lib.* surface:
PLY read (lib/ply.py instead of open3d), voxelisation (lib.sparse.voxelize instead of ME.sparse_quantize,
pairwise_demo.py:61-98), PairwiseReg.compute_descriptors (FCGF -> sampling -> feature NN) and
filter_correspondences (OANet -> Procrustes).  --visualize needs open3d, which is absent: it is reported
and skipped.

usage: python -m scripts.pairwise_demo configs/pairwise_registration/demo/config.yaml \
           [--source_pc ...cloud_bin_0.ply] [--target_pc ...cloud_bin_1.ply] [--model pairwise_reg.pt] [--verbose]

--fpfh registers the pair without any network or checkpoint (lib/fpfh.py): voxel centroids at the
config's voxel_size, normals oriented to each cloud's mean, FPFH descriptors, mutual feature matches, RANSAC and,
with --icp, a point-to-point ICP refinement; T is printed and written to the same est_T.log.  --fpfh --fgr runs Fast
Global Registration (lib.fpfh.register_fgr) on the matches in place of RANSAC.  --fpfh --iss matches
the descriptors of ISS keypoints only (FragmentOverlap.iss_keypoints).
    [--fpfh [--fpfh_radius R] [--normal_radius R] [--checkers | --fgr] [--iss] [--icp]]   (defaults: 5 and 2 voxel sizes)
"""
import argparse
import logging
import os
import sys
import time

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import lib.config as config  # noqa: E402
from lib.checkpoints import CheckpointIO  # noqa: E402
from lib.ply import read_ply_xyz  # noqa: E402
from lib.sparse import voxelize  # noqa: E402
from lib.utils import load_config, write_trajectory  # noqa: E402


def prepare_data(point_cloud_files, voxel_size, device):
    """pairwise_demo.py:61-98: voxel-downsampled clouds + the batched sparse input of FCGF"""
    raw = [read_ply_xyz(f) for f in point_cloud_files]
    coords, _, counts, xyz_down = voxelize(raw, voxel_size, device)
    return {"pcd0": xyz_down, "sinput0_C": coords, "sinput0_F": torch.ones(coords.shape[0], 1, device=device),
            "pts_list": torch.tensor(counts)}


def _write(est_T, args):
    """est_T.log in the reference's place -> its path"""
    target_base = "./data/demo/pairwise/results"
    id_0 = args.source_pc.split(os.sep)[-1].split("_")[-1].split(".")[0]
    id_1 = args.target_pc.split(os.sep)[-1].split("_")[-1].split(".")[0]
    os.makedirs(target_base, exist_ok=True)
    target_path = os.path.join(target_base, "est_T.log")
    write_trajectory(np.expand_dims(est_T, 0), [[id_0, id_1, "True"]], target_path)
    return target_path


def main_fpfh(cfg, args, logger=logging.getLogger()):
    """--fpfh: FPFH + RANSAC or FGR (+ ICP) on the two clouds' voxel centroids; no model, no checkpoint"""
    from lib.fpfh import register_fgr, register_fpfh
    from lib.icp import icp_refine
    from lib.overlap import FragmentOverlap
    voxel = float(cfg["misc"]["voxel_size"])
    r_fpfh = 5.0 * voxel if args.fpfh_radius is None else args.fpfh_radius
    r_normal = 2.0 * voxel if args.normal_radius is None else args.normal_radius
    if not (r_fpfh > 0.0 and r_normal > 0.0):
        raise ValueError("--fpfh_radius and --normal_radius must be positive")
    t0 = time.time()
    raw = [read_ply_xyz(f) for f in (args.source_pc, args.target_pc)]
    fo = FragmentOverlap(raw, "FCGF", voxel, radius=max(r_fpfh, r_normal))
    xyz = fo.xyz.cpu().numpy()
    fo.estimate_normals(r_normal, viewpoints=[xyz[fo.off[b]:fo.off[b + 1]].mean(0) for b in range(2)])
    fo.compute_fpfh(r_fpfh)
    fgr = bool(getattr(args, "fgr", False))
    kp = {}
    if getattr(args, "iss", False):   # register_scene's radii: 3 and 2 voxel sizes, where the index allows them
        kp = {"keypoints": fo.iss_keypoints(min(fo.r, 3.0 * voxel), min(fo.r, 2.0 * voxel))}
    if fgr:
        out = register_fgr(fo, [[0, 1]], **kp)
    else:
        out = register_fpfh(fo, [[0, 1]], checkers=bool(getattr(args, "checkers", False)), **kp)
    if kp:
        print("ISS: %d / %d keypoints of %d / %d points" % (out["n_keypoints"][0, 0], out["n_keypoints"][0, 1],
                                                            fo.off[1], fo.off[2] - fo.off[1]))
    if "n_pass" in out:
        logger.info("checkers: %d of 100000 samples passed, %d scored", out["n_pass"][0], out["n_valid"][0])
    est_T = out["T"][0]
    logger.info("FPFH + %s: %d mutual matches of %d / %d points, fitness %.4f, rmse %.4f", "FGR" if fgr else "RANSAC",
                out["n_matches"][0], fo.off[1], fo.off[2] - fo.off[1], out["fitness"][0], out["rmse"][0])
    if fgr:
        print("FGR: fitness %.4f, rmse %.4f over %d mutual matches (%d tuples, status %d)"
              % (out["fitness"][0], out["rmse"][0], out["n_matches"][0], out["n_tuples"][0], out["status"][0]))
    if args.icp:
        ref = icp_refine(fo, [[0, 1]], est_T[None], max_dist=min(fo.r, 2.0 * voxel))
        est_T = ref["T"][0]
        logger.info("ICP: %d iterations, fitness %.4f, rmse %.4f", ref["iters"][0], ref["fitness"][0], ref["rmse"][0])
    target_path = _write(est_T, args)
    print("T (source -> target):\n%s" % np.array2string(est_T, precision=8, suppress_small=True))
    if args.verbose:
        logger.info("Registration without a network completed in %.3fs", time.time() - t0)
        logger.info("Estimated parameters were saved in %s.", target_path)
    return est_T


def check_args(args):
    """ValueError for --fgr or --iss without --fpfh, and for --fgr with --checkers"""
    if getattr(args, "iss", False) and not getattr(args, "fpfh", False):
        raise ValueError("--iss picks the points whose FPFH descriptors are matched: it needs --fpfh")
    if getattr(args, "fgr", False):
        if not getattr(args, "fpfh", False):
            raise ValueError("--fgr registers the FPFH matches: it needs --fpfh")
        if getattr(args, "checkers", False):
            raise ValueError("--checkers belongs to RANSAC: not with --fgr")
    return args


def main(cfg, args, logger=logging.getLogger()):
    check_args(args)
    if getattr(args, "fpfh", False):
        return main_fpfh(cfg, args, logger)
    np.random.seed(41)     # pairwise_demo.py:25-28 (the Sampler draws on numpy's global RandomState)
    torch.manual_seed(41)
    model = config.get_model(cfg)
    model.eval()
    ckpt = CheckpointIO("", initialize_from="./pretrained/", initialization_file_name=args.model, model=model)
    try:
        ckpt.load()
    except FileExistsError:
        logger.warning("no pretrained model %s: random-init weights", args.model)
    logger.info("Total number of model parameters: %d", sum(p.numel() for p in model.parameters()))
    target_base = "./data/demo/pairwise/results"
    id_0 = args.source_pc.split(os.sep)[-1].split("_")[-1].split(".")[0]
    id_1 = args.target_pc.split(os.sep)[-1].split("_")[-1].split(".")[0]
    os.makedirs(target_base, exist_ok=True)
    target_path = os.path.join(target_base, "est_T.log")
    dev = torch.device("cuda")
    with torch.no_grad():
        t0 = time.time()
        data = prepare_data([args.source_pc, args.target_pc], cfg["misc"]["voxel_size"], dev)
        t1 = time.time()
        filtering_data, _, _ = model.compute_descriptors(data)
        t2 = time.time()
        est = model.filter_correspondences(filtering_data)
        est_T = np.eye(4)
        est_T[0:3, 0:3] = est["rot_est"][-1].cpu().numpy()
        est_T[0:3, 3:4] = est["trans_est"][-1].cpu().numpy()
        t3 = time.time()
    write_trajectory(np.expand_dims(est_T, 0), [[id_0, id_1, "True"]], target_path)
    if args.verbose:
        logger.info("Feature computation and sampling took %.3fs", t2 - t1)
        logger.info("Filtering the correspondences and estimation of paramaters took %.3fs", t3 - t2)
        logger.info("Estimation of the pairwise transformation parameters completed in %.3fs", t3 - t0)
        logger.info("Estimated parameters were saved in %s.", target_path)
    if args.visualize:
        logger.warning("--visualize needs open3d (not available): skipped")
    return est_T


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", default="./configs/pairwise_registration/demo/config.yaml", type=str, help="config file")
    ap.add_argument("--source_pc", default="./data/demo/pairwise/raw_data/cloud_bin_0.ply", type=str)
    ap.add_argument("--target_pc", default="./data/demo/pairwise/raw_data/cloud_bin_1.ply", type=str)
    ap.add_argument("--model", default="pairwise_reg.pt", type=str, help="Name of the pretrained model.")
    ap.add_argument("--verbose", action="store_true", help="Write out the intermediate results and timings")
    ap.add_argument("--visualize", action="store_true", help="Visualize the point cloud and the results.")
    ap.add_argument("--fpfh", action="store_true", help="Register with FPFH + RANSAC: no network, no checkpoint.")
    ap.add_argument("--fpfh_radius", default=None, type=float, help="FPFH support radius (default 5 voxel sizes).")
    ap.add_argument("--normal_radius", default=None, type=float, help="Normal radius (default 2 voxel sizes).")
    ap.add_argument("--checkers", action="store_true",
                    help="With --fpfh: RANSAC with edge-length and distance checkers, 3-point samples, 100000 draws.")
    ap.add_argument("--fgr", action="store_true",
                    help="With --fpfh: Fast Global Registration on the matches instead of RANSAC (not with --checkers).")
    ap.add_argument("--iss", action="store_true",
                    help="With --fpfh: match the descriptors of ISS keypoints only (Open3D's compute_iss_keypoints).")
    ap.add_argument("--icp", action="store_true", help="With --fpfh: refine the estimate by point-to-point ICP.")
    return ap


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(name)s - %(message)s")
    a = parser().parse_args()
    main(load_config(a.config), a)
