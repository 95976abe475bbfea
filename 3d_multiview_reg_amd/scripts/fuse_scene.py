"""Fuse a scene's registered fragments into one cloud: poses.txt + fragment PLYs -> scene.ply.

Reads the `poses.txt` scripts/multiview_sync.py (or scripts/register_scene.py) writes (one block per fragment:
`i i N` and the 4 x 4 pose M_i, fragment i -> the anchor's frame) and the fragments' PLY files, fragment i of
--fragments being block i; maps every fragment by its pose and merges the points per voxel on the GPU
(lib.multiview.fuse_scene, csrc/fuse.hip): the place of Open3D's `pcd_combined += pcd.transform(pose)`,
voxel_down_sample and write_point_cloud.  With --normals the fragments' normals are estimated first (radius
--normal_radius, oriented towards each fragment's own origin, where its sensor stood) and fused with the points.

usage: python -m scripts.fuse_scene --poses DIR/poses.txt --fragments F0.ply F1.ply ... --voxel_size 0.025
           [--min_frags 2] [--normals --normal_radius 0.075] --out scene.ply
"""
import argparse
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from lib.ply import read_ply_xyz, write_ply  # noqa: E402
from lib.utils import read_trajectory  # noqa: E402


def read_poses(filename, n_fragments):
    """poses.txt -> [n,4,4]; block i must be fragment i of n"""
    keys, poses = read_trajectory(filename)
    if len(poses) != n_fragments or any(int(k[0]) != i or int(k[1]) != i for i, k in enumerate(keys)):
        raise ValueError("%s holds %d poses; expected the blocks `i i N` of %d fragments in order"
                         % (filename, len(poses), n_fragments))
    return poses


def fuse_fragments(xyz_list, poses, voxel_size, min_frags=1, normals=False, normal_radius=None):
    """xyz_list: the fragments' points; poses [n,4,4] -> the dict of lib.multiview.fuse_scene over the raw points.
    normals: estimated over normal_radius (None: 3 voxel_size) with every fragment's origin as its viewpoint."""
    from lib.multiview import fuse_scene
    from lib.overlap import FragmentOverlap
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    radius = 3.0 * float(voxel_size) if normal_radius is None else float(normal_radius)
    fo = FragmentOverlap(xyz_list, "3DMatch", radius=radius)
    if normals:
        fo.estimate_normals(radius, np.zeros((len(xyz_list), 3)))
    return fuse_scene(fo, poses[:, :3, :3], poses[:, :3, 3], voxel_size, min_frags=min_frags)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--poses", required=True, help="poses.txt: one 4 x 4 pose per fragment (fragment -> scene)")
    ap.add_argument("--fragments", required=True, nargs="+", help="the fragments' PLY files, fragment i = block i")
    ap.add_argument("--voxel_size", type=float, required=True, help="edge of the voxels the points are merged in")
    ap.add_argument("--min_frags", type=int, default=1, help="keep the voxels at least so many fragments fell into")
    ap.add_argument("--normals", action="store_true", help="estimate, fuse and write normals as well")
    ap.add_argument("--normal_radius", type=float, default=None, help="--normals: the radius of the normal "
                    "estimation (default 3 voxel_size)")
    ap.add_argument("--out", required=True, help="the fused cloud (PLY)")
    return ap


def check_args(ap, a):
    if not a.voxel_size > 0.0:
        ap.error("--voxel_size must be positive")
    if a.min_frags < 1:
        ap.error("--min_frags must be at least 1")
    if a.normal_radius is not None and not a.normals:
        ap.error("--normal_radius goes with --normals")
    if a.normal_radius is not None and not a.normal_radius > 0.0:
        ap.error("--normal_radius must be positive")
    return a


def main(argv=None):
    ap = parser()
    a = check_args(ap, ap.parse_args(argv))
    frags = [read_ply_xyz(f) for f in a.fragments]
    poses = read_poses(a.poses, len(frags))
    scene = fuse_fragments(frags, poses, a.voxel_size, a.min_frags, a.normals, a.normal_radius)
    out_dir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(out_dir, exist_ok=True)
    write_ply(a.out, scene["xyz"].cpu().numpy(), None if scene["normals"] is None else scene["normals"].cpu().numpy())
    nf = scene["n_frags"].cpu().numpy()
    print("fused %d fragments (%d points) into %d voxels of %g (seen by %.2f fragments on average, %d by one only) "
          "-> %s" % (len(frags), sum(len(f) for f in frags), len(nf), a.voxel_size, nf.mean() if len(nf) else 0.0,
                     int((nf == 1).sum()), a.out))
    return scene


if __name__ == "__main__":
    main()
