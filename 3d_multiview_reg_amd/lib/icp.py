"""Fine registration: batched ICP on the fragments' own points, point-to-point (csrc/icp.hip mvr_icp_refine,
DESIGN.md 4.19), point-to-plane on normals (csrc/icp_plane.hip mvr_icp_refine_plane) or generalized,
plane-to-plane, on both fragments' normals (csrc/icp_gicp.hip mvr_icp_refine_generalized); the
semantics are in include/mvreg.h; coloured ICP on both the geometry and the fragments' colours is a fourth
(csrc/icp_colored.hip mvr_icp_refine_colored).  Each of them takes a robust kernel (`kernel`,
`kernel_k`: csrc/icp_robust.hip mvr_icp_refine_robust), which weighs every correspondence by its
residual in the solve.

The reference stops at the coarse estimate (Procrustes or RANSAC over the sampled correspondences); its users
follow it with Open3D's `registration_icp`.  `icp_refine` does that for every pair of a scene in one launch, on the
radius index a `FragmentOverlap` already holds; `icp_pair` keeps the one-pair shape of `registration_icp`.
`gicp_refine` and `gicp_pair` are the same two shapes for `registration_generalized_icp`, `colored_icp_refine` and
`colored_icp_pair` for `registration_colored_icp`.  Restated from the maths and pinned to tests/icp_oracle.py,
tests/icp_plane_oracle.py, tests/gicp_oracle.py, tests/icp_robust_oracle.py and tests/colored_icp_oracle.py: Open3D
parity is unpinned.

Convention: T maps source coordinates into the target's frame, x_target ~ R x_source + t (rot_est / trans_est of
filter_correspondences, the input of lib.multiview.synchronize) — the inverse of the `trans` of
FragmentOverlap.ratios."""
import numpy as np
import torch

from lib import _native as N
from lib.overlap import _point_tensor

STATUS_FEW_CORRESPONDENCES, STATUS_ITERATION_CAP, STATUS_INVALID_PAIR = 1, 2, 4
# the 6 x 6 system is not positive definite to working precision; point-to-point: only with a robust kernel, when the
# weights of the correspondences do not sum to more than 0 (every residual beyond Tukey's k)
STATUS_DEGENERATE = 8
METHODS = ("point_to_point", "point_to_plane")
ROBUST_KERNELS = ("l2", "huber", "cauchy", "gm", "tukey")       # MVR_KERNEL_*: the index is the C constant
_METHOD_IDS = {"point_to_point": 0, "point_to_plane": 1, "generalized": 2}                  # MVR_ICP_*


def _check_settings(name, max_dist, max_iters, tol_fitness, tol_rmse):
    if not max_dist > 0.0:
        raise ValueError("%s: max_dist must be positive" % name)
    if int(max_iters) < 0:
        raise ValueError("%s: max_iters must not be negative" % name)
    if not (tol_fitness >= 0.0 and tol_rmse >= 0.0):
        raise ValueError("%s: the tolerances must not be negative" % name)


def _check_method(name, method):
    if method not in METHODS:
        raise ValueError("%s: method must be one of %s, not %r" % (name, ", ".join(METHODS), method))


def _check_epsilon(name, epsilon):
    if not 0.0 < epsilon <= 1.0:
        raise ValueError("%s: epsilon must lie in (0, 1]" % name)


def _check_kernel(name, kernel, kernel_k, return_weight_sum=False):
    """-> None for the plain entry, or (MVR_KERNEL_* id, k) for mvr_icp_refine_robust"""
    if kernel is None:
        if kernel_k is not None:
            raise ValueError("%s: kernel_k needs a kernel" % name)
        if return_weight_sum:
            raise ValueError("%s: return_weight_sum needs a kernel ('l2' gives the count)" % name)
        return None
    if kernel not in ROBUST_KERNELS:
        raise ValueError("%s: kernel must be one of %s, not %r" % (name, ", ".join(ROBUST_KERNELS), kernel))
    if kernel == "l2":
        return 0, 0.0 if kernel_k is None else float(kernel_k)
    if kernel_k is None or not float(kernel_k) > 0.0:
        raise ValueError("%s: kernel %r needs a positive kernel_k" % (name, kernel))
    return ROBUST_KERNELS.index(kernel), float(kernel_k)


def _run(name, fo, pairs, T_in, T_name, max_dist, needs_normals, call, normals_for=""):
    """The marshalling every batched entry shares: max_dist against fo.r, T_in [P,4,4] / [P,3,4] and pairs [P,2] to
    fp64 / int64 on fo's device, fo.normals checked when needs_normals (normals_for: what needs them, for the
    message), then call(P, pairs, T3) -> dict of device tensors.  The dict comes back on the device when T_in was
    there, else on the host (numpy for numpy inputs)."""
    if max_dist > fo.r:
        raise ValueError("%s: max_dist %g exceeds the index's cell size %g (build the FragmentOverlap with "
                         "radius >= max_dist)" % (name, max_dist, fo.r))
    Tin = torch.as_tensor(T_in)
    if Tin.dim() != 3 or tuple(Tin.shape[1:]) not in ((4, 4), (3, 4)) or not Tin.is_floating_point():
        raise ValueError("%s: %s must be a float [P,4,4] or [P,3,4]" % (name, T_name))
    ij = torch.as_tensor(pairs)
    if ij.dim() != 2 or ij.shape[1] != 2 or ij.shape[0] != Tin.shape[0]:
        raise ValueError("%s: pairs must be [P,2] with one row per transform" % name)
    if needs_normals:
        nrm = getattr(fo, "normals", None)
        if nrm is None:
            raise ValueError("%s: %sneeds fo.normals (call fo.estimate_normals())" % (name, normals_for))
        _point_tensor(name, "normals", nrm, (fo.M, 3), fo.xyz)
    N.require_hip()
    return N.hand_back(call(int(Tin.shape[0]), ij.to(fo.device, torch.int64).contiguous(),
                            Tin[:, :3, :].to(fo.device, torch.float64).contiguous()), T_in)


def _refine(name, fo, pairs, T_init, max_dist, max_iters, tol_fitness, tol_rmse, return_trace, entry, needs_normals,
            normals_for="", epsilon=None, robust=None, return_weight_sum=False, lambda_geometric=None):
    """icp_refine, gicp_refine and colored_icp_refine after their own checks: entry names the C function, which takes
    the normals when needs_normals and epsilon when that is not None.  robust (_check_kernel's pair) not None:
    mvr_icp_refine_robust as the method `entry` names, with w_sum when return_weight_sum.  lambda_geometric not None:
    mvr_icp_refine_colored, which takes fo.intensity and fo.color_grad after the normals and robust's pair and w_sum as
    the robust entry does."""
    def call(P, ij, T0):
        dev = fo.device
        T = torch.empty(P, 3, 4, dtype=torch.float64, device=dev)
        fitness, rmse = (torch.empty(P, dtype=torch.float64, device=dev) for _ in range(2))
        n_corr, iters, status = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
        trace = torch.empty(P, int(max_iters) + 1, 2, dtype=torch.float64, device=dev) if return_trace else None
        w_sum = torch.empty(P, dtype=torch.float64, device=dev) if return_weight_sum else None
        nrm = (N.ptr(fo.normals),) if needs_normals else ()
        pairs_in = (N.ptr(ij), N.ptr(T0), P)
        settings = (int(max_iters), float(tol_fitness), float(tol_rmse))
        outs = (N.ptr(T), N.ptr(fitness), N.ptr(rmse), N.ptr(n_corr), N.ptr(iters), N.ptr(status), N.ptr(trace))
        if lambda_geometric is not None:
            fn, args = "mvr_icp_refine_colored", (
                *fo._points(), *nrm, N.ptr(fo.intensity), N.ptr(fo.color_grad), *fo._fragments(), *pairs_in, max_dist,
                float(lambda_geometric), *robust, *settings, *outs, N.ptr(w_sum))
        elif robust is not None:
            fn, args = "mvr_icp_refine_robust", (
                *fo._points(), *(nrm or (None,)), *fo._fragments(), *pairs_in, _METHOD_IDS[entry], max_dist,
                1.0 if epsilon is None else float(epsilon), *robust, *settings, *outs, N.ptr(w_sum))
        else:
            eps = () if epsilon is None else (float(epsilon),)
            fn, args = entry, (*fo._points(), *nrm, *fo._fragments(), *pairs_in, max_dist, *eps, *settings, *outs)
        N.check(getattr(N.lib(), fn)(*args, N.stream()), fn)
        T4 = torch.zeros(P, 4, 4, dtype=torch.float64, device=dev)
        T4[:, :3], T4[:, 3, 3] = T, 1.0
        out = {"T": T4, "fitness": fitness, "rmse": rmse, "n_corr": n_corr, "iters": iters, "status": status}
        if return_trace:
            out["trace"] = trace
        if return_weight_sum:
            out["w_sum"] = w_sum
        return out
    return _run(name, fo, pairs, T_init, "T_init", max_dist, needs_normals, call, normals_for)


def _pair_overlap(name, src_xyz, tgt_xyz, T_init, max_dist, voxel_size, normal_radius, normals, colors=None):
    """The shape checks of icp_pair, gicp_pair and colored_icp_pair, then the two-fragment FragmentOverlap (with
    normals over normal_radius, None: max_dist, if asked for; with colors, a pair of [n,3] arrays, also the colour
    gradients over it) and T_init with the leading [1]."""
    from lib.overlap import FragmentOverlap
    if normal_radius is not None and not normal_radius > 0.0:
        raise ValueError("%s: normal_radius must be positive" % name)
    if voxel_size is not None and not voxel_size > 0.0:
        raise ValueError("%s: voxel_size must be positive" % name)
    for what, x in (("src_xyz", src_xyz), ("tgt_xyz", tgt_xyz)):
        shape = tuple(x.shape) if torch.is_tensor(x) else np.shape(x)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError("%s: %s must be [n,3]" % (name, what))
    Tin = torch.as_tensor(T_init)
    if tuple(Tin.shape) not in ((4, 4), (3, 4)) or not Tin.is_floating_point():
        raise ValueError("%s: T_init must be a float [4,4] or [3,4]" % name)
    nr = max_dist if normal_radius is None else normal_radius
    cell = max(max_dist, nr) if normals else max_dist    # the index's cells cover the search ball and the normals'
    with_colors = {} if colors is None else {"colors": colors}
    if voxel_size is None:
        fo = FragmentOverlap([src_xyz, tgt_xyz], "3DMatch", radius=cell, **with_colors)
    else:
        fo = FragmentOverlap([src_xyz, tgt_xyz], "FCGF", voxel_size, radius=cell, **with_colors)
    if normals:
        fo.estimate_normals(nr)
    if colors is not None:
        fo.compute_color_gradients(nr)
    return fo, (T_init[None] if torch.is_tensor(T_init) else np.asarray(T_init)[None])


def icp_refine(fo, pairs, T_init, max_dist=None, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6, return_trace=False,
               method="point_to_point", kernel=None, kernel_k=None, return_weight_sum=False):
    """Refine the transform of every pair on the points of `fo` (a lib.overlap.FragmentOverlap: its centroids for
    method 'FCGF', its raw points for '3DMatch').

    pairs [P,2] (source, target) fragment indices; T_init [P,4,4] or [P,3,4], numpy or torch, any float dtype;
    max_dist: the correspondence distance, at most fo.r (None: fo.r).  Stops after max_iters solves, or when fitness
    and rmse both change by less than their tolerances (absolute); both tolerances 0 run exactly max_iters.
    method 'point_to_plane' minimises the distances along the target's normals instead: fo.normals (fp64 [M,3] on the
    device, from fo.estimate_normals() or assigned by the caller) must be there; their sign does not matter.
    kernel: one of ROBUST_KERNELS, with its scale kernel_k > 0 in the unit of the residual (metres; 'gm': metres
    squared; 'l2' takes none).  Every correspondence then enters the solve with the weight w(r) of its residual
    (include/mvreg.h mvr_icp_refine_robust): the distance, or for 'point_to_plane' the distance along the normal.
    Fitness, rmse, n_corr and the stopping rule stay unweighted.  return_weight_sum adds fp64 w_sum [P], the weights'
    sum at the returned T.  None: the plain loop, every weight 1.
    Returns a dict of fp64 T [P,4,4], fp64 fitness / rmse [P], int32 n_corr / iters / status [P] (STATUS_* bits) and,
    with return_trace, fp64 trace [P, max_iters + 1, 2]: (fitness, rmse) of every evaluation, -1 after the last.
    The outputs stay on the device when T_init was on the device; otherwise they come back on the host (numpy for
    numpy inputs)."""
    max_dist = float(fo.r if max_dist is None else max_dist)
    _check_settings("icp_refine", max_dist, max_iters, tol_fitness, tol_rmse)
    _check_method("icp_refine", method)
    robust = _check_kernel("icp_refine", kernel, kernel_k, return_weight_sum)
    plane = method == "point_to_plane"
    if robust is not None:
        return _refine("icp_refine", fo, pairs, T_init, max_dist, max_iters, tol_fitness, tol_rmse, return_trace,
                       method, plane, "method 'point_to_plane' ", robust=robust, return_weight_sum=return_weight_sum)
    return _refine("icp_refine", fo, pairs, T_init, max_dist, max_iters, tol_fitness, tol_rmse, return_trace,
                   "mvr_icp_refine_plane" if plane else "mvr_icp_refine", plane, "method 'point_to_plane' ")


INFO_ORDERS = ("redwood", "open3d")
_OPEN3D_PERM = (3, 4, 5, 0, 1, 2)


def permute_information(info, order="open3d"):
    """Swap the translation and rotation blocks of information matrices [..., 6, 6]: (v, omega) <-> (omega, v).  The
    permutation is its own inverse; order 'redwood' returns the input."""
    if order not in INFO_ORDERS:
        raise ValueError("permute_information: order must be one of %s, not %r" % (", ".join(INFO_ORDERS), order))
    if order == "redwood":
        return info
    p = list(_OPEN3D_PERM)
    return info[..., p, :][..., :, p]


def information_matrix(fo, pairs, T, max_dist=None, order="redwood"):
    """The 6 x 6 information matrix of every pair at its transform, on the points of `fo` (csrc/info.hip
    mvr_pair_information): sum G^T G over the correspondences eval(T) of icp_refine finds, G =
    [I | -[y]x] at the matched target point y.  What Open3D's get_information_matrix_from_point_clouds(source,
    target, max_dist, T) gives a pose-graph edge; Open3D parity is unpinned.

    pairs [P,2] (source, target); T [P,4,4] or [P,3,4] with x_target ~ T x_source, numpy or torch, any float dtype;
    max_dist at most fo.r (None: fo.r).  order 'redwood': parameters (translation, rotation), the order of a Redwood
    .info file, of lib.utils.computeTransformationErr and of lib.multiview.optimize_pose_graph, info[:, 0, 0] ==
    n_corr; 'open3d': (rotation, translation), Open3D's.
    Returns a dict of fp64 info [P,6,6], int32 n_corr [P], fp64 rmse [P], int32 status [P] (0, or
    STATUS_INVALID_PAIR with a zero matrix).  The outputs stay on the device when T was on the device; otherwise they
    come back on the host (numpy for numpy inputs)."""
    max_dist = float(fo.r if max_dist is None else max_dist)
    if not max_dist > 0.0:
        raise ValueError("information_matrix: max_dist must be positive")
    if order not in INFO_ORDERS:
        raise ValueError("information_matrix: order must be one of %s, not %r" % (", ".join(INFO_ORDERS), order))

    def call(P, ij, T3):
        info = torch.empty(P, 36, dtype=torch.float64, device=fo.device)
        rmse = torch.empty(P, dtype=torch.float64, device=fo.device)
        n_corr, status = (torch.empty(P, dtype=torch.int32, device=fo.device) for _ in range(2))
        N.check(N.lib().mvr_pair_information(*fo._points(), *fo._fragments(), N.ptr(ij), N.ptr(T3), P, max_dist,
                                             N.ptr(info), N.ptr(n_corr), N.ptr(rmse), N.ptr(status), N.stream()),
                "mvr_pair_information")
        return {"info": permute_information(info.view(P, 6, 6), order), "n_corr": n_corr, "rmse": rmse,
                "status": status}
    return _run("information_matrix", fo, pairs, T, "T", max_dist, False, call)


def icp_pair(src_xyz, tgt_xyz, T_init, max_dist=0.05, voxel_size=None, method="point_to_point", normal_radius=None,
             **kw):
    """One pair in the shape of Open3D's registration_icp(source, target, max_correspondence_distance, init):
    src_xyz [n,3], tgt_xyz [m,3], T_init [4,4] or [3,4] with x_target ~ T x_source.  voxel_size None: the raw points;
    a value: Open3D-style voxel centroids of both clouds (lib.overlap).  **kw: max_iters, tol_fitness, tol_rmse,
    return_trace, kernel, kernel_k, return_weight_sum of icp_refine.  method 'point_to_plane': the normals are
    estimated here over normal_radius (None: max_dist) on an index of cell max(max_dist, normal_radius);
    TransformationEstimationPointToPlane after
    estimate_normals(KDTreeSearchParamRadius(normal_radius)).  Returns icp_refine's dict without the leading [P]."""
    _check_settings("icp_pair", float(max_dist), kw.get("max_iters", 30), kw.get("tol_fitness", 0.0),
                    kw.get("tol_rmse", 0.0))
    _check_method("icp_pair", method)
    _check_kernel("icp_pair", kw.get("kernel"), kw.get("kernel_k"), kw.get("return_weight_sum", False))
    fo, T0 = _pair_overlap("icp_pair", src_xyz, tgt_xyz, T_init, max_dist, voxel_size, normal_radius,
                           method == "point_to_plane")
    out = icp_refine(fo, [[0, 1]], T0, max_dist, method=method, **kw)
    return {k: v[0] for k, v in out.items()}


def gicp_refine(fo, pairs, T_init, max_dist=None, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6, epsilon=1e-3,
                return_trace=False, kernel=None, kernel_k=None, return_weight_sum=False):
    """Generalized (plane-to-plane) ICP on every pair of `fo`: icp_refine's arguments, conventions, stopping rule and
    dict, with the solve of Segal et al.'s GICP (Open3D's registration_generalized_icp; parity unpinned).

    Every point's covariance is 1 in its surface and `epsilon` along its normal, so both fragments' surfaces weigh a
    residual.  fo.normals (fp64 [M,3] on the device, from fo.estimate_normals() or assigned by the caller) must be
    there and unit: they are not renormalised, their sign does not matter.  epsilon in (0, 1]; 1 makes the normals
    drop out.  status bit STATUS_DEGENERATE as for 'point_to_plane'.  kernel, kernel_k, return_weight_sum: as
    icp_refine's, on the residual sqrt(d^T A d) (d = q - y, A the inverse of the pair's summed covariances: a distance
    in which the surfaces' own directions count half, so roughly metres)."""
    max_dist = float(fo.r if max_dist is None else max_dist)
    _check_settings("gicp_refine", max_dist, max_iters, tol_fitness, tol_rmse)
    _check_epsilon("gicp_refine", epsilon)
    robust = _check_kernel("gicp_refine", kernel, kernel_k, return_weight_sum)
    if robust is not None:
        return _refine("gicp_refine", fo, pairs, T_init, max_dist, max_iters, tol_fitness, tol_rmse, return_trace,
                       "generalized", True, epsilon=epsilon, robust=robust, return_weight_sum=return_weight_sum)
    return _refine("gicp_refine", fo, pairs, T_init, max_dist, max_iters, tol_fitness, tol_rmse, return_trace,
                   "mvr_icp_refine_generalized", True, epsilon=epsilon)


def gicp_pair(src_xyz, tgt_xyz, T_init, max_dist=0.05, voxel_size=None, normal_radius=None, epsilon=1e-3, **kw):
    """One pair in the shape of Open3D's registration_generalized_icp(source, target, max_correspondence_distance,
    init): icp_pair's arguments.  The normals of both clouds are estimated here over normal_radius (None: max_dist) on
    an index of cell max(max_dist, normal_radius).  **kw: max_iters, tol_fitness, tol_rmse, return_trace, kernel,
    kernel_k, return_weight_sum of gicp_refine.  Returns gicp_refine's dict without the leading [P]."""
    _check_settings("gicp_pair", float(max_dist), kw.get("max_iters", 30), kw.get("tol_fitness", 0.0),
                    kw.get("tol_rmse", 0.0))
    _check_epsilon("gicp_pair", epsilon)
    _check_kernel("gicp_pair", kw.get("kernel"), kw.get("kernel_k"), kw.get("return_weight_sum", False))
    fo, T0 = _pair_overlap("gicp_pair", src_xyz, tgt_xyz, T_init, max_dist, voxel_size, normal_radius, True)
    out = gicp_refine(fo, [[0, 1]], T0, max_dist, epsilon=epsilon, **kw)
    return {k: v[0] for k, v in out.items()}


def _check_lambda(name, lambda_geometric):
    if not 0.0 <= lambda_geometric <= 1.0:
        raise ValueError("%s: lambda_geometric must lie in [0, 1]" % name)


def _check_colored(name, fo):
    """the per-point inputs of the coloured loop: fp64, on the device, in the row order of fo.xyz; what is missing is
    named (the normals are looked at again by _run)"""
    for what, hint in (("normals", "fo.estimate_normals()"), ("intensity", "fo.compute_color_gradients()"),
                       ("color_grad", "fo.compute_color_gradients()")):
        x = getattr(fo, what, None)
        if x is None:
            raise ValueError("%s: needs fo.%s (call %s)" % (name, what, hint))
        shape = (fo.M,) if what == "intensity" else (fo.M, 3)
        _point_tensor(name, what, x, shape, fo.xyz, str(list(shape)))


def colored_icp_refine(fo, pairs, T_init, max_dist=None, max_iters=30, tol_fitness=1e-6, tol_rmse=1e-6,
                       lambda_geometric=0.968, kernel=None, kernel_k=None, return_trace=False,
                       return_weight_sum=False):
    """Coloured ICP on every pair of `fo`: icp_refine's arguments, conventions, stopping rule and dict, with the solve
    of Park, Zhou and Koltun's coloured ICP (Open3D's registration_colored_icp; parity unpinned).

    Every correspondence adds the point-to-plane term with the share lambda_geometric and, with the share
    1 - lambda_geometric, a photometric term: the source point's intensity against the target's intensity and its
    gradient in the tangent plane.  Where the geometry leaves a motion free (in the plane of a wall, a floor, a table
    top) the colours decide it.  Needs fo.normals (from fo.estimate_normals() or assigned by the caller; taken as
    given, their sign does not matter) and fo.intensity and fo.color_grad (from fo.compute_color_gradients(), or
    assigned by the caller: fp64 [M] and [M,3] on the device).  lambda_geometric in [0, 1]; 1 is the point-to-plane
    solve.  status bit STATUS_DEGENERATE as for 'point_to_plane'.  kernel, kernel_k: as icp_refine's, applied to each
    of the two residuals scaled by the root of its share (metres for the geometric one, intensity for the photometric
    one); None and 'l2' are the same launch.  return_weight_sum adds fp64 w_sum [P], the sum of lambda_geometric w_G +
    (1 - lambda_geometric) w_I at the returned T (without a kernel: n_corr)."""
    max_dist = float(fo.r if max_dist is None else max_dist)
    _check_settings("colored_icp_refine", max_dist, max_iters, tol_fitness, tol_rmse)
    _check_lambda("colored_icp_refine", float(lambda_geometric))
    robust = _check_kernel("colored_icp_refine", kernel, kernel_k, return_weight_sum and kernel is not None)
    if max_dist <= fo.r:       # beyond it _run raises
        _check_colored("colored_icp_refine", fo)
    return _refine("colored_icp_refine", fo, pairs, T_init, max_dist, max_iters, tol_fitness, tol_rmse, return_trace,
                   "mvr_icp_refine_colored", True, robust=robust or (0, 0.0), return_weight_sum=return_weight_sum,
                   lambda_geometric=lambda_geometric)


def colored_icp_pair(src_xyz, src_colors, tgt_xyz, tgt_colors, T_init, max_dist=0.05, voxel_size=None,
                     normal_radius=None, lambda_geometric=0.968, **kw):
    """One pair in the shape of Open3D's registration_colored_icp(source, target, max_correspondence_distance, init):
    icp_pair's arguments plus the two clouds' colours [n,3] / [m,3] (float in [0, 1] or uint8).  The normals and the
    colour gradients of both clouds are estimated here over normal_radius (None: max_dist) on an index of cell
    max(max_dist, normal_radius).  **kw: max_iters, tol_fitness, tol_rmse, return_trace, kernel, kernel_k,
    return_weight_sum of colored_icp_refine.  Returns colored_icp_refine's dict without the leading [P]."""
    _check_settings("colored_icp_pair", float(max_dist), kw.get("max_iters", 30), kw.get("tol_fitness", 0.0),
                    kw.get("tol_rmse", 0.0))
    _check_lambda("colored_icp_pair", float(lambda_geometric))
    _check_kernel("colored_icp_pair", kw.get("kernel"), kw.get("kernel_k"),
                  kw.get("return_weight_sum", False) and kw.get("kernel") is not None)
    fo, T0 = _pair_overlap("colored_icp_pair", src_xyz, tgt_xyz, T_init, max_dist, voxel_size, normal_radius, True,
                           colors=[src_colors, tgt_colors])
    out = colored_icp_refine(fo, [[0, 1]], T0, max_dist, lambda_geometric=lambda_geometric, **kw)
    return {k: v[0] for k, v in out.items()}
