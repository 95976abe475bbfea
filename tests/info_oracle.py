"""numpy restatement of the per-pair information matrix (csrc/info.hip mvr_pair_information).

    correspondences: those of icp_oracle.evaluate(src, tgt, T, max_dist) — nearest target point y of q = R x + t,
                     valid iff |q - y| < max_dist (strict)
    G_y  = [ I3 | -[y]x ]                       (3 x 6; parameters (translation v, rotation omega))
    info = sum over the valid correspondences of G_y^T G_y

The sum is taken literally, matrix by matrix: the kernel assembles the same thing from ten moments (n, sum y,
sum y y^T), so an assembly error there shows up against this.  Open3D is absent: parity with its
get_information_matrix_from_point_clouds (the same G, blocks in (omega, v) order) is unpinned.
"""
import functools

import numpy as np

import icp_oracle


def skew(y):
    return np.array([[0.0, -y[2], y[1]], [y[2], 0.0, -y[0]], [-y[1], y[0], 0.0]])


def information_from_points(ys):
    """sum G_y^T G_y over the rows of ys [n,3] -> [6,6]"""
    ys = np.asarray(ys, np.float64).reshape(-1, 3)
    G = np.zeros((len(ys), 3, 6))
    G[:, :, :3] = np.eye(3)
    for k, y in enumerate(ys):
        G[k, :, 3:] = -skew(y)
    return np.einsum("nki,nkj->ij", G, G)   # sum_n G_n^T G_n


def information(src, tgt, T, max_dist):
    """One pair -> dict(info [6,6], n_corr, rmse, gap, edge, ys [n_corr,3])"""
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    ev = icp_oracle.evaluate(src, tgt, np.asarray(T, np.float64), max_dist)
    ys = tgt[ev["idx"][ev["valid"]]] if ev["n_corr"] else np.zeros((0, 3))
    return {"info": information_from_points(ys), "n_corr": ev["n_corr"], "rmse": ev["rmse"], "gap": ev["gap"],
            "edge": ev["edge"], "ys": ys}


def information_batch(frags, pairs, T, max_dist):
    """The batch as mvr_pair_information sees it; an invalid pair comes out with status 4 and a zero matrix"""
    out = []
    for (s, g), Tp in zip(np.asarray(pairs).reshape(-1, 2), np.asarray(T, np.float64)):
        if not (0 <= s < len(frags) and 0 <= g < len(frags)) or not np.all(np.isfinite(Tp[:3])):
            out.append({"info": np.zeros((6, 6)), "n_corr": 0, "rmse": 0.0, "gap": np.inf, "edge": np.inf,
                        "ys": np.zeros((0, 3)), "status": 4})
        else:
            out.append(dict(information(frags[s], frags[g], Tp, max_dist), status=0))
    return out


OPEN3D_PERM = [3, 4, 5, 0, 1, 2]


def to_open3d(info):
    """(v, omega) <-> (omega, v): an involution"""
    return np.asarray(info)[..., OPEN3D_PERM, :][..., :, OPEN3D_PERM]


# --------------------------------------------------------------------------------------------------- the test cases
SIZES = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025)


def small_case_all_sizes():
    """icp_oracle.small_case with sources of 1023 and 1024 points (the first rows of the 1025-point one) and an empty
    fragment that serves as a target: every size of SIZES, the far-away source, and the pair (3 points -> empty)"""
    frags, pairs, T0 = icp_oracle.small_case()
    big = len(icp_oracle.SMALL_SIZES)            # fragment index of the 1025-point source
    assert len(frags[big]) == 1025
    frags = list(frags) + [frags[big][:1023], frags[big][:1024], np.zeros((0, 3))]
    n = len(frags)
    pairs = np.concatenate([pairs, [[n - 3, 0], [n - 2, 0], [4, n - 1]]])
    T0 = np.concatenate([T0, T0[big - 1:big], T0[big - 1:big], T0[3:4]])
    return frags, pairs, T0


@functools.lru_cache(maxsize=None)
def cases():
    """(name, fragments as the oracle sees them, pairs, T, max_dist): test_info_host.py checks their margins,
    test_gpu_info.py runs them"""
    cent = icp_oracle.scene4_centroids()
    poses = icp_oracle.scene4()[1]
    out = [("centroids", cent, np.asarray(icp_oracle.TWELVE), icp_oracle.eval_starts(cent), 0.075),
           ("centroids_0.03", cent, np.asarray(icp_oracle.TWELVE), icp_oracle.eval_starts(cent), 0.03)]
    src, tgt, T0, max_dist, _ = icp_oracle.pair_case()
    out.append(("pair", [src, tgt], np.asarray([[0, 1], [0, 1]]),
                np.stack([T0, icp_oracle.gt_transform(poses, 0, 1)]), max_dist))
    frags, pairs, T = small_case_all_sizes()
    out.append(("small", frags, pairs, T, icp_oracle.SMALL_MAX_DIST))
    ctgt, Tt, Ts = icp_oracle.full_copy_case(cent[0])
    out.append(("full_copy", [cent[0], ctgt], np.asarray([[0, 1], [0, 1]]), np.stack([Ts, Tt]), 0.05))
    return tuple(out)
