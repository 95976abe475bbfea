"""Multiview stage: one globally consistent pose per fragment from a scene's pairwise estimates.

`synchronize` is the transformation synchronisation of the paper's sections 3.2-3.3 (closed-form weighted solve:
an eigenproblem for the rotations, a linear solve for the translations) with optional IRLS, on the GPU
(csrc/sync.hip mvr_sync_poses; the maths and the conventions are in DESIGN.md 4.18).  The
reference never released this stage, so there is no reference module behind this file.
`optimize_pose_graph` refines those poses over SE(3) (csrc/posegraph.hip); both take a batch of scenes
through one marshaller, `_scene_batch`, as their kernels share csrc/scene.hpp.  `fuse_scene` maps the
fragments by the poses and merges the points per voxel into the registered scene (csrc/fuse.hip mvr_fuse_scene,
DESIGN.md 4.25), and `register_scene` composes the library's stages from fragments to that scene without a pretrained
network.

Conventions: edge k = (i, j) with x_j ~ R_k x_i + t_k (source i, target j: lib.utils.pair_index order, the rot_est /
trans_est of filter_correspondences); pose (R_i, t_i) maps fragment i into the anchor's frame, X = R_i x_i + t_i.
"""
from types import SimpleNamespace

import numpy as np
import torch

from lib import _native as N

STATUS_NOT_CONNECTED, STATUS_ITERATION_CAP, STATUS_EDGE_IGNORED = 1, 2, 4
MAX_FRAGS = 128   # include/mvreg.h MVR_SYNC_MAX_FRAGS


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else None


FLAG = "flag"   # a field's dtype: anything comparable with 0, kept as int32 (non-zero -> 1)


def _field(x, dtype, dev):
    x = torch.as_tensor(x)
    return (x.to(dev) != 0).to(torch.int32) if dtype == FLAG else x.to(dev, dtype)


def _scene_batch(name, edge_fields, frag_fields, n_frags, n_edges, anchor, like):
    """The marshalling `synchronize` and `optimize_pose_graph` share: a batch of scenes, each an edge list over its
    fragments, in one of three forms -> padded contiguous tensors.

    edge_fields / frag_fields: (label, value, trailing shape, dtype, optional) per array with one row per edge / per
    fragment; the first of each gives the count (frag_fields may be empty: n_frags then gives the fragments).  dtype
    torch.float64, torch.int32 or FLAG; an optional field may be None and stays None.  The forms: one scene (values
    [E, ...]), per-scene lists of such, or a padded batch ([S, E, ...]) with n_frags / n_edges [S] (defaults: all).
    like: the argument that decides the placement: the tensors go to its device when it is on one (else to the
    current HIP device, or stay on the host when there is none: the rules can be checked without a device) and
    finish() hands the outputs back where it was (N.hand_back).
    Every broken rule is a ValueError.  Returns a namespace of x (label -> [S, count, ...] or None), S, Fmax, Emax, the
    host lists nf, ne, their int32 device copies n_f, n_e, dev, and finish(dict of [S, ...] tensors)."""
    lists = _as_list(like)
    first = like if lists is None else (like[0] if lists else torch.zeros(0))
    if torch.is_tensor(first) and first.device.type == "cuda":
        dev = first.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    groups = (("pose", "F", frag_fields), ("edge", "E", edge_fields))
    for _, _, fields in groups:
        for label, value, _, _, optional in fields:
            if value is None and not optional:
                raise ValueError("%s: %s is required" % (name, label))
    x, counts, sizes = {}, {}, {}
    if lists is not None:   # per-scene lists -> padded
        S = len(lists)
        if any(_as_list(v) is None or len(v) != S for _, _, fs in groups for _, v, _, _, _ in fs if v is not None):
            raise ValueError("%s: the per-scene lists must have one entry per scene" % name)
        for what, _, fields in groups:
            for label, value, tail, dtype, _ in fields:
                if value is None:
                    x[label] = None
                    continue
                per, rows = int(np.prod(tail, dtype=np.int64)), []
                for s in range(S):
                    v = _field(value[s], dtype, dev)
                    if v.numel() % per or (what in counts and v.numel() // per != counts[what][s]):
                        raise ValueError("%s: scene %d: one %s per %s" % (name, s, label, what))
                    rows.append(v.reshape((v.numel() // per,) + tail))
                counts.setdefault(what, [int(r.shape[0]) for r in rows])
                sizes[what] = max(counts[what] + [0])
                x[label] = torch.zeros((S, sizes[what]) + tail, dtype=torch.int32 if dtype == FLAG else dtype,
                                       device=dev)
                for s in range(S):
                    x[label][s, :counts[what][s]] = rows[s]
    else:
        S = batched = None
        for what, sym, fields in groups:
            for k, (label, value, tail, dtype, _) in enumerate(fields):
                if value is None:
                    x[label] = None
                    continue
                v = _field(value, dtype, dev)
                if k == 0:   # the field that gives the count
                    if v.dim() < len(tail) + 1 or tuple(v.shape[v.dim() - len(tail):]) != tail or \
                            v.dim() - len(tail) not in ((1, 2) if batched is None else (2 if batched else 1,)):
                        shape = ",".join([sym] + [str(d) for d in tail])
                        raise ValueError("%s: %s must be [%s] or [S,%s]%s" % (
                            name, label, shape, shape, "" if batched is None else ", as %s is" % like_label))
                    if batched is None:
                        batched, like_label = v.dim() - len(tail) == 2, label
                    v = v if batched else v.unsqueeze(0)
                    if S is not None and v.shape[0] != S:
                        raise ValueError("%s: %s and %s must hold the same scenes" % (name, like_label, label))
                    S, sizes[what] = int(v.shape[0]), int(v.shape[1])
                else:
                    try:
                        v = v.reshape((S, sizes[what]) + tail)
                    except RuntimeError:
                        raise ValueError("%s: %s must be given one %sper %s"
                                         % (name, label, "row " if what == "pose" else "", what)) from None
                x[label] = v.contiguous()

        def given(n, most, what, sym):
            c = [most] * S if n is None else [int(v) for v in torch.as_tensor(n).reshape(-1).tolist()]
            if len(c) != S or min(c + [0]) < 0 or max(c + [0]) > most:
                raise ValueError("%s: %s must be [S] with 0 <= %s <= %s" % (name, what, what, sym))
            return c
        counts["edge"] = given(n_edges, sizes["edge"], "n_edges", "E")
        if frag_fields:
            counts["pose"] = given(n_frags, sizes["pose"], "n_frags", "F")
    if not frag_fields:   # the fragments are counted, not given
        counts["pose"] = [int(v) for v in torch.as_tensor(n_frags).reshape(-1).tolist()]
        if len(counts["pose"]) != S or min(counts["pose"] + [0]) < 0:
            raise ValueError("%s: n_frags must give one count per scene, none negative" % name)
        sizes["pose"] = max(counts["pose"] + [0])
    if sizes["pose"] > MAX_FRAGS:
        raise ValueError("%s: at most %d fragments per scene" % (name, MAX_FRAGS))
    if not 0 <= int(anchor) < max(sizes["pose"], 1):
        raise ValueError("%s: anchor outside the fragments" % name)
    single = lists is None and not batched
    return SimpleNamespace(x=x, S=S, Fmax=sizes["pose"], Emax=sizes["edge"], nf=counts["pose"], ne=counts["edge"],
                           n_f=torch.tensor(counts["pose"], dtype=torch.int32).to(dev),
                           n_e=torch.tensor(counts["edge"], dtype=torch.int32).to(dev), dev=dev,
                           finish=lambda out: N.hand_back(out, first, single))


def _edge_fields(R_pair, t_pair, pairs, weights):
    """_scene_batch's per-edge fields of both entries"""
    return (("R_pair", R_pair, (3, 3), torch.float64, False), ("t_pair", t_pair, (3,), torch.float64, False),
            ("pair", pairs, (2,), torch.int32, False), ("weight", weights, (), torch.float64, True))


def synchronize(R_pair, t_pair, pairs, n_frags, weights=None, anchor=0, irls_iters=0, c_rot=0.1, c_trans=0.1,
                n_edges=None):
    """Poses of every fragment from pairwise estimates (batched over scenes, one launch).

    One scene: R_pair [E,3,3], t_pair [E,3] (or [E,3,1]), pairs [E,2], n_frags int, weights [E] or None (all ones).
    A batch: lists of such per-scene arrays with n_frags a list, or padded R_pair [S,E,3,3], t_pair [S,E,3],
    pairs [S,E,2], weights [S,E] with n_frags [S] and n_edges [S] (default E for every scene).
    Inputs are torch tensors or numpy arrays, fp32 or fp64; the solve is fp64.  A shape or a count that breaks these
    rules is a ValueError, raised before a device is asked for.
    Returns a dict of fp64 R [N,3,3], t [N,3], int32 member [N], fp64 weights / res_rot / res_trans [E] (the last
    IRLS pass's weights and per-edge residuals) and int32 status (bits: 1 some fragment is not connected to the
    anchor and came out as identity with member 0, 2 an eigen-solve hit its iteration cap, 4 an edge was ignored or
    the scene is invalid); a batch adds a leading [S] (padded to the largest N and E).  The outputs stay on the
    device when R_pair was on the device; otherwise they come back on the host (numpy for numpy inputs)."""
    b = _scene_batch("synchronize", _edge_fields(R_pair, t_pair, pairs, weights), (), n_frags, n_edges, anchor, R_pair)
    N.require_hip()
    S, Fmax, Emax, dev = b.S, b.Fmax, b.Emax, b.dev
    # the rows past a scene's n_frags: identity as well
    R = torch.eye(3, dtype=torch.float64, device=dev).repeat(S, Fmax, 1, 1)
    t = torch.zeros(S, Fmax, 3, dtype=torch.float64, device=dev)
    member = torch.zeros(S, Fmax, dtype=torch.int32, device=dev)
    w_out, res_rot, res_trans = (torch.zeros(S, Emax, dtype=torch.float64, device=dev) for _ in range(3))
    status = torch.zeros(S, dtype=torch.int32, device=dev)
    if S and Fmax:
        L = N.lib()
        ws = N.workspace(L.mvr_sync_workspace_bytes(S, Fmax, Emax), dev)
        N.check(L.mvr_sync_poses(N.ptr(b.x["R_pair"]), N.ptr(b.x["t_pair"]), N.ptr(b.x["pair"]), N.ptr(b.x["weight"]),
                                 Emax, N.ptr(b.n_e), N.ptr(b.n_f), S, Fmax, Emax, int(anchor), int(irls_iters),
                                 float(c_rot), float(c_trans), N.ptr(R), N.ptr(t), Fmax, N.ptr(member), N.ptr(w_out),
                                 N.ptr(res_rot), N.ptr(res_trans), N.ptr(status), N.ptr(ws), ws.numel(), N.stream()),
                "mvr_sync_poses")
    return b.finish({"R": R, "t": t, "member": member, "weights": w_out, "res_rot": res_rot, "res_trans": res_trans,
                     "status": status})


PG_STATUS_NOT_CONNECTED, PG_STATUS_ITERATION_CAP, PG_STATUS_EDGE_IGNORED, PG_STATUS_FACTORISATION = 1, 2, 4, 8
PG_STATUS_LINE_PROCESS_OFF = 16


def optimize_pose_graph(R, t, R_pair, t_pair, pairs, info, weights=None, anchor=0, max_iters=20, lambda0=1e-6,
                        tol_cost=1e-9, tol_step=1e-10, return_trace=False, n_frags=None, n_edges=None,
                        line_process=False, uncertain=None, preference_loop_closure=1.0,
                        max_correspondence_distance=None, edge_prune_threshold=0.25, prune_passes=2):
    """Refine poses jointly over SE(3) with per-edge information matrices (batched over scenes, one launch;
    csrc/posegraph.hip mvr_posegraph_optimize): Levenberg-Marquardt on sum_k w_k xi_k^T info_k xi_k,
    xi_k = (v, omega) of M_j^-1 M_i T_k^-1, from the poses `synchronize` returns, the anchor held.  The stage of
    Open3D's global_optimization; Open3D parity is unpinned.  Without line_process there is no robust kernel: a
    wrong edge is held back only by its weight.

    One scene: R [N,3,3], t [N,3] (the initial poses), R_pair [E,3,3], t_pair [E,3] (or [E,3,1]), pairs [E,2],
    info [E,6,6] (or [E,36]) in the (translation, rotation) order of lib.icp.information_matrix, weights [E] or None
    (all ones; e.g. the IRLS weights `synchronize` returned).  A batch: lists of such per-scene arrays, or padded
    R [S,F,3,3], t [S,F,3], R_pair [S,E,3,3], t_pair [S,E,3], pairs [S,E,2], info [S,E,6,6], weights [S,E] with
    n_frags [S] and n_edges [S] (defaults F and E for every scene).  torch tensors or numpy arrays, fp32 or fp64.
    A trial solves (H + lambda diag H) delta = -g; a lower cost accepts it (lambda / 10), otherwise lambda * 10.
    Stops after max_iters trials, after an accepted trial that lowered the cost by at most tol_cost (relative), or
    after a trial with max|delta| <= tol_step.
    Returns a dict of fp64 R [N,3,3], t [N,3], int32 member [N], fp64 cost [2] (initial, final), int32 iters and
    status (PG_STATUS_* bits) and, with return_trace, fp64 trace [max_iters + 1]: the cost at the start and after
    every trial, -1 after the last; a batch adds a leading [S].  The outputs stay on the device when R was on the
    device; otherwise they come back on the host (numpy for numpy inputs).

    line_process=True is Open3D's global_optimization with its line process and edge pruning (mvr_posegraph_optimize_lp,
    DESIGN.md 4.22a; tests/posegraph_lp_oracle.py is the normative text): every uncertain edge (uncertain [E] /
    [S,E] / per-scene list, non-zero = a loop closure; None: every edge) carries a weight l = (mu / (mu + r))^2,
    r = w xi^T info xi, mu = preference_loop_closure * max_correspondence_distance^2 * the mean info[0, 0] of the
    uncertain edges; max_correspondence_distance (the distance the information matrices were built with) is then
    required.  prune_passes times: optimise, give the uncertain edges with l < edge_prune_threshold weight 0,
    continue from the result (Open3D does this twice); prune_passes=0 is one optimisation without pruning.  The dict
    is the last pass's (cost [2]: that pass's initial and final cost) and adds fp64 line [E] (the l of the last pass
    in which the edge counted, 1 for a certain edge, 0 for one that never counted), bool kept [E] (False: pruned),
    fp64 mu (the last pass's) and passes: a list of per-pass dicts of iters, status and cost.  Status bit
    PG_STATUS_LINE_PROCESS_OFF: mu was not positive and finite, the pass ran with l = 1."""
    if int(max_iters) < 0:
        raise ValueError("optimize_pose_graph: max_iters must not be negative")
    if line_process:
        if max_correspondence_distance is None:
            raise ValueError("optimize_pose_graph: line_process needs max_correspondence_distance, the distance the "
                             "information matrices were built with")
        mu_scale = float(preference_loop_closure) * float(max_correspondence_distance) ** 2
        if not (mu_scale > 0.0 and mu_scale < float("inf")):
            raise ValueError("optimize_pose_graph: preference_loop_closure and max_correspondence_distance must be "
                             "finite and positive")
        if not 0.0 <= float(edge_prune_threshold) <= 1.0:
            raise ValueError("optimize_pose_graph: edge_prune_threshold must lie in [0, 1]")
        if int(prune_passes) < 0:
            raise ValueError("optimize_pose_graph: prune_passes must not be negative")
    if not (float(lambda0) >= 0.0 and float(lambda0) < float("inf")):
        raise ValueError("optimize_pose_graph: lambda0 must be finite and not negative")
    if not (tol_cost >= 0.0 and tol_step >= 0.0):
        raise ValueError("optimize_pose_graph: the tolerances must not be negative")
    b = _scene_batch("optimize_pose_graph",
                     _edge_fields(R_pair, t_pair, pairs, weights) + (
                         ("info", info, (36,), torch.float64, False),
                         ("uncertain flag", uncertain if line_process else None, (), FLAG, True)),
                     (("R", R, (3, 3), torch.float64, False), ("t", t, (3,), torch.float64, False)),
                     n_frags, n_edges, anchor, R)
    N.require_hip()
    S, Fmax, Emax, dev = b.S, b.Fmax, b.Emax, b.dev
    Rp, tp, ij, w, lam, unc, R0, t0 = (b.x[k] for k in ("R_pair", "t_pair", "pair", "weight", "info",
                                                         "uncertain flag", "R", "t"))
    Ro, to = R0.clone(), t0.clone()      # the rows past a scene's n_frags keep their input
    member = torch.zeros(S, Fmax, dtype=torch.int32, device=dev)
    cost = torch.zeros(S, 2, dtype=torch.float64, device=dev)
    iters, status = (torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2))
    out = {"R": Ro, "t": to, "member": member, "cost": cost, "iters": iters, "status": status}
    if return_trace:
        out["trace"] = torch.full((S, int(max_iters) + 1), -1.0, dtype=torch.float64, device=dev)
    trace = out.get("trace")
    L = N.lib() if S and Fmax else None      # nothing to launch otherwise
    if not line_process:
        if L is not None:
            ws = N.workspace(L.mvr_posegraph_workspace_bytes(S, Fmax, Emax), dev)
            N.check(L.mvr_posegraph_optimize(
                N.ptr(Rp), N.ptr(tp), N.ptr(ij), N.ptr(w), N.ptr(lam), Emax, N.ptr(b.n_e), N.ptr(b.n_f), S, Fmax, Emax,
                int(anchor), N.ptr(R0), N.ptr(t0), int(max_iters), float(lambda0), float(tol_cost), float(tol_step),
                N.ptr(Ro), N.ptr(to), Fmax, N.ptr(member), N.ptr(cost), N.ptr(iters), N.ptr(status), N.ptr(trace),
                N.ptr(ws), ws.numel(), N.stream()), "mvr_posegraph_optimize")
        return b.finish(out)
    line = torch.zeros(S, Emax, dtype=torch.float64, device=dev)
    kept = torch.ones(S, Emax, dtype=torch.bool, device=dev)
    mu = torch.zeros(S, dtype=torch.float64, device=dev)
    passes = []
    w = torch.ones(S, Emax, dtype=torch.float64, device=dev) if w is None else w.clone()
    flag = torch.ones(S, Emax, dtype=torch.bool, device=dev) if unc is None else unc != 0
    live = torch.arange(Emax, device=dev)[None, :] < b.n_e[:, None].to(torch.int64)
    for p in range(max(int(prune_passes), 1)):
        if p:
            R0, t0 = Ro.clone(), to.clone()
        l_p = torch.zeros(S, Emax, dtype=torch.float64, device=dev)
        if L is not None:
            ws = N.workspace(L.mvr_posegraph_lp_workspace_bytes(S, Fmax, Emax), dev)
            N.check(L.mvr_posegraph_optimize_lp(
                N.ptr(Rp), N.ptr(tp), N.ptr(ij), N.ptr(w), N.ptr(lam), N.ptr(unc), Emax, N.ptr(b.n_e), N.ptr(b.n_f), S,
                Fmax, Emax, int(anchor), N.ptr(R0), N.ptr(t0), int(max_iters), float(lambda0), float(tol_cost),
                float(tol_step), mu_scale, N.ptr(Ro), N.ptr(to), Fmax, N.ptr(member), N.ptr(cost), N.ptr(iters),
                N.ptr(status), N.ptr(trace), N.ptr(l_p), N.ptr(mu), N.ptr(ws), ws.numel(), N.stream()),
                "mvr_posegraph_optimize_lp")
        passes.append({"iters": iters.clone(), "status": status.clone(), "cost": cost.clone()})
        counted = (l_p > 0.0) & live             # a counted edge's l is positive (1 for a certain one)
        line = torch.where(counted, l_p, line)
        if int(prune_passes) > 0:
            drop = counted & flag & (l_p < float(edge_prune_threshold))
            w = torch.where(drop, torch.zeros_like(w), w)
            kept &= ~drop
    out = b.finish(dict(out, line=line, kept=kept, mu=mu))
    out["passes"] = [b.finish(p) for p in passes]
    return out


def _poses4(R, t):
    R = torch.as_tensor(R)
    t = torch.as_tensor(t).to(R).reshape(R.shape[0], 3)
    M = torch.zeros(R.shape[0], 4, 4, dtype=R.dtype, device=R.device)
    M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = R, t, 1.0
    return M


def pairwise_from_poses(R, t, pairs):
    """The synchronised pairwise estimates T [E,4,4], T_k = M_j^-1 M_i for pairs[k] = (i, j): the same convention as
    synchronize's inputs (x_j ~ T_k x_i).  R [N,3,3], t [N,3], pairs [E,2]; torch in, torch out (same device and
    dtype as R); numpy in, numpy out."""
    was_numpy = not torch.is_tensor(R)
    M = _poses4(R, t)
    ij = torch.as_tensor(pairs).to(M.device, torch.long).reshape(-1, 2)
    Mi, Mj = M[ij[:, 0]], M[ij[:, 1]]
    Rjt = Mj[:, :3, :3].transpose(1, 2)
    T = torch.zeros(ij.shape[0], 4, 4, dtype=M.dtype, device=M.device)
    T[:, :3, :3] = Rjt @ Mi[:, :3, :3]
    T[:, :3, 3] = (Rjt @ (Mi[:, :3, 3] - Mj[:, :3, 3]).unsqueeze(-1)).squeeze(-1)
    T[:, 3, 3] = 1.0
    return T.numpy() if was_numpy else T


def weights_from_scores(scores, threshold=0.5):
    """Edge weights from the filtering network's scores [P, n] (the final block's, out["scores"][-1]): per pair, the
    share of correspondences whose score exceeds `threshold`.  A heuristic that stands in for the paper's learned
    pair confidence — it is not a reproduction of it.  One expression on the scores' device."""
    return (scores > threshold).to(torch.float64).mean(dim=-1)


MAX_FUSE_VOXELS_PER_AXIS = (1 << 21) - 1   # largest 21-bit voxel index of mvr_fuse_scene (include/mvreg.h)


def _fuse_arguments(B, R, t, voxel_size, member, min_frags, min_points):
    """fuse_scene's checks that need no device -> (R [B,3,3], t [B,3], member [B] or None) as torch tensors where
    they were"""
    if not (float(voxel_size) > 0.0 and float(voxel_size) < float("inf")):
        raise ValueError("fuse_scene: voxel_size must be positive and finite")
    if int(min_frags) < 1 or int(min_points) < 1:
        raise ValueError("fuse_scene: min_frags and min_points must be at least 1")
    R, t = torch.as_tensor(R), torch.as_tensor(t)
    if tuple(R.shape) != (B, 3, 3) or not R.is_floating_point():
        raise ValueError("fuse_scene: R must be a float [%d,3,3], one rotation per fragment" % B)
    if tuple(t.shape) not in ((B, 3), (B, 3, 1)) or not t.is_floating_point():
        raise ValueError("fuse_scene: t must be a float [%d,3] (or [%d,3,1]), one translation per fragment" % (B, B))
    if not (bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all())):
        raise ValueError("fuse_scene: R and t must be finite")
    if member is not None:
        member = torch.as_tensor(member)
        if tuple(member.shape) != (B,) or member.is_floating_point() or member.is_complex():
            raise ValueError("fuse_scene: member must be a bool or integer [%d], one flag per fragment" % B)
    return R, t.reshape(B, 3), member


def fuse_scene(fo, R, t, voxel_size, member=None, min_frags=1, min_points=1, normals=None):
    """The registered scene as one cloud (csrc/fuse.hip mvr_fuse_scene): the points of `fo` (a
    lib.overlap.FragmentOverlap) mapped by the fragments' poses and merged per voxel of `voxel_size`.  The place of
    Open3D's `pcd_combined += pcd.transform(pose)` and voxel_down_sample; Open3D parity is unpinned.

    R [B,3,3], t [B,3] (or [B,3,1]): pose of every fragment, X = R_b x + t_b (what synchronize and
    optimize_pose_graph return), numpy or torch, any float dtype.  member [B] (bool or integer, None: all): a zero
    leaves the fragment out (pass the `member` synchronize returned).  normals None: fo.normals when it is set;
    False: fuse without normals; a contiguous fp64 [M,3] device tensor: those.  Normals are averaged as they are, so
    their orientation matters (fo.estimate_normals(viewpoints=...)).
    min_frags / min_points keep the voxels that at least so many distinct fragments / points fell into (a voxel seen
    by one fragment only is the usual sign of a misregistered fragment or of clutter); the rows are filtered on the
    device.
    Returns a dict of xyz fp64 [V,3] (device; ascending voxel key), normals fp64 [V,3] or None, n_points and n_frags
    int32 [V], voxel_size."""
    R, t, member = _fuse_arguments(fo.B, R, t, voxel_size, member, min_frags, min_points)
    nrm = getattr(fo, "normals", None) if normals is None else (None if normals is False else normals)
    if nrm is not None and (not torch.is_tensor(nrm) or tuple(nrm.shape) != (fo.M, 3) or nrm.dtype != torch.float64
                            or nrm.device != fo.xyz.device or not nrm.is_contiguous()):
        raise ValueError("fuse_scene: normals must be a contiguous fp64 [%d,3] tensor on the device of fo.xyz" % fo.M)
    N.require_hip()
    dev, M, voxel = fo.device, int(fo.M), float(voxel_size)
    poses = torch.cat([R.to(dev, torch.float64), t.to(dev, torch.float64).unsqueeze(-1)], 2).reshape(fo.B, 12)
    poses = poses.contiguous()
    mem = None if member is None else (member != 0).to(dev, torch.uint8).contiguous()
    cap = max(M, 1)
    xyz = torch.empty(cap, 3, dtype=torch.float64, device=dev)
    out_n = torch.empty(cap, 3, dtype=torch.float64, device=dev) if nrm is not None else None
    n_points, n_frags = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
    count = torch.empty(1, dtype=torch.int64, device=dev)
    L = N.lib()
    ws_b = L.mvr_fuse_scene_workspace_bytes(M)
    ws = N.workspace(ws_b, dev)
    N.check(L.mvr_fuse_scene(N.ptr(fo.xyz), N.ptr(nrm), N.ptr(fo.off_dev), fo.B, M, N.ptr(poses), N.ptr(mem), voxel,
                             N.ptr(ws), ws_b, N.ptr(xyz), N.ptr(out_n), N.ptr(n_points), N.ptr(n_frags),
                             N.ptr(count), N.stream()), "mvr_fuse_scene")
    V = int(count.item())   # set on the device by mvr_fuse_scene: no synchronisation beyond this copy
    if V < 0:
        raise ValueError("fuse_scene: the posed scene spans more than %d voxels of size %g along an axis (voxel "
                         "indices are 21-bit, so an extent of at most %g), or a mapped point is not finite; use a "
                         "larger voxel_size or leave the stray fragment out with `member`"
                         % (MAX_FUSE_VOXELS_PER_AXIS, voxel, MAX_FUSE_VOXELS_PER_AXIS * voxel))
    xyz, n_points, n_frags = xyz[:V], n_points[:V], n_frags[:V]
    out_n = None if out_n is None else out_n[:V]
    if int(min_frags) > 1 or int(min_points) > 1:
        keep = (n_frags >= int(min_frags)) & (n_points >= int(min_points))
        xyz, n_points, n_frags = xyz[keep], n_points[keep], n_frags[keep]
        out_n = None if out_n is None else out_n[keep]
    return {"xyz": xyz, "normals": out_n, "n_points": n_points, "n_frags": n_frags, "voxel_size": voxel}


OVERLAP_THRESHOLDS = {"3d_match": 0.3, "redwood": 0.23}   # scripts/benchmark_pairwise_registration.py --dataset
ICP_METHODS = ("point_to_point", "point_to_plane", "generalized", "colored")


def _scene_arguments(n, voxel_size, method, dataset, init, viewpoints, colors=None, icp_lambda_geometric=0.968):
    """register_scene's checks that need no device -> (pairs [P,2], init [P,4,4] or None, viewpoints [n,3])"""
    if n < 2:
        raise ValueError("register_scene: needs at least two fragments")
    if n > MAX_FRAGS:
        raise ValueError("register_scene: at most %d fragments per scene" % MAX_FRAGS)
    if not (float(voxel_size) > 0.0 and float(voxel_size) < float("inf")):
        raise ValueError("register_scene: voxel_size must be positive and finite")
    if method not in ICP_METHODS:
        raise ValueError("register_scene: method must be one of %s, not %r" % (", ".join(ICP_METHODS), method))
    if method == "colored" and colors is None:
        raise ValueError("register_scene: method 'colored' needs colors, one [n_b,3] array per fragment")
    if colors is not None and len(colors) != n:
        raise ValueError("register_scene: colors must hold one array per fragment (%d, not %d)" % (n, len(colors)))
    if not 0.0 <= float(icp_lambda_geometric) <= 1.0:
        raise ValueError("register_scene: icp_lambda_geometric must lie in [0, 1]")
    if dataset not in OVERLAP_THRESHOLDS:
        raise ValueError("register_scene: dataset must be one of %s, not %r"
                         % (", ".join(sorted(OVERLAP_THRESHOLDS)), dataset))
    pairs = np.asarray([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int64)
    if init is not None:
        init = np.asarray(init, dtype=np.float64)
        if init.shape != (len(pairs), 4, 4) or not np.isfinite(init).all():
            raise ValueError("register_scene: init must hold a finite 4 x 4 estimate for each of the %d pairs i < j, "
                             "in that order" % len(pairs))
    viewpoints = np.zeros((n, 3)) if viewpoints is None else np.asarray(viewpoints, dtype=np.float64)
    if viewpoints.shape != (n, 3) or not np.isfinite(viewpoints).all():
        raise ValueError("register_scene: viewpoints must be a finite [%d,3], one per fragment" % n)
    return pairs, init, viewpoints


COARSE_METHODS = ("ransac", "fgr")   # register_scene's step 4: lib.fpfh.register_fpfh / register_fgr
DENOISE_METHODS = {"statistical": {"nb_neighbors": 20, "std_ratio": 2.0}, "radius": {"nb_points": 16, "radius": None},
                   "cluster": {"min_points": 10, "min_size": 100, "eps": None}}


def _denoise_arguments(denoise, r=None):
    """register_scene's checks of `denoise` that need no device (r: the index's cell size, where it is known) ->
    None, or a dict of "method" and that method's options with the defaults filled in"""
    from lib.overlap import _radius_outlier_arguments, _statistical_arguments
    if denoise is None:
        return None
    if not isinstance(denoise, dict) or "method" not in denoise:
        raise ValueError("register_scene: denoise must be None or a dict with a 'method'")
    method = denoise["method"]
    if method not in DENOISE_METHODS:
        raise ValueError("register_scene: denoise method must be one of %s, not %r"
                         % (", ".join(sorted(DENOISE_METHODS)), method))
    unknown = sorted(set(denoise) - set(DENOISE_METHODS[method]) - {"method"})
    if unknown:
        raise ValueError("register_scene: denoise method %r has no option %s" % (method, ", ".join(map(repr, unknown))))
    d = dict(DENOISE_METHODS[method], **denoise)
    if method == "statistical":
        d["nb_neighbors"], d["std_ratio"] = _statistical_arguments(d["nb_neighbors"], d["std_ratio"])
    elif method == "cluster":
        from lib.overlap import _cluster_keep_arguments, _dbscan_arguments
        rr = float("inf") if r is None else float(r)
        eps, d["min_points"] = _dbscan_arguments(d["eps"], d["min_points"], rr)
        d["eps"] = None if d["eps"] is None else eps
        d["min_size"] = _cluster_keep_arguments(d["min_size"], False)[0]
    else:
        rr = float("inf") if r is None else float(r)
        d["nb_points"], radius = _radius_outlier_arguments(d["nb_points"], rr if d["radius"] is None else d["radius"],
                                                           rr)
        d["radius"] = None if d["radius"] is None else radius
    return d


def _keypoints_arguments(keypoints, r=None, init=None):
    """register_scene's checks of `keypoints` that need no device (r: the index's cell size, where it is known) ->
    None, or a dict of "match" and iss_keypoints' options with the defaults filled in (a radius left None stays
    None)"""
    from lib.fpfh import KEYPOINT_MATCH
    from lib.overlap import ISS_DEFAULTS, _iss_arguments
    if keypoints is None:
        return None
    if keypoints is not True and not isinstance(keypoints, dict):
        raise ValueError("register_scene: keypoints must be None, True or a dict of iss_keypoints' options and 'match'")
    if init is not None:
        raise ValueError("register_scene: keypoints belong to the coarse registration, which init replaces")
    given = {} if keypoints is True else keypoints
    unknown = sorted(set(given) - set(ISS_DEFAULTS) - {"match"})
    if unknown:
        raise ValueError("register_scene: keypoints has no option %s" % ", ".join(map(repr, unknown)))
    d = dict(dict(ISS_DEFAULTS, match="keypoints"), **given)
    if d["match"] not in KEYPOINT_MATCH:
        raise ValueError("register_scene: keypoints 'match' must be one of %s, not %r"
                         % (", ".join(KEYPOINT_MATCH), d["match"]))
    rr = float("inf") if r is None else float(r)
    checked = _iss_arguments(*[d[k] for k in ISS_DEFAULTS], rr)
    for k, v in zip(ISS_DEFAULTS, checked):
        if d[k] is not None:
            d[k] = v
    return d


def register_scene(xyz_list, voxel_size=0.025, method="point_to_point", init=None, viewpoints=None, downsample=True,
                   dataset="3d_match", overlap_threshold=None, normal_radius=None, fpfh_radius=None, seed=0,
                   icp_max_dist=None, icp_iters=30, gicp_epsilon=1e-3, anchor=0, refine_iters=20, fuse_voxel=None,
                   min_frags=1, min_points=1, ransac_checkers=False, line_process=False,
                   preference_loop_closure=1.0, denoise=None, coarse="ransac", keypoints=None, icp_kernel=None,
                   icp_kernel_k=None, colors=None, icp_lambda_geometric=0.968):
    """Fragments in, registered scene out, without a pretrained network: the chain of the stages this library has,
    composed (nothing is computed here).  xyz_list: n point arrays [n_b,3] in their own frames.
      1. lib.overlap.FragmentOverlap: voxel centroids of size voxel_size on an index of radius 3 voxel_size
         (downsample False: the points as given on the same index); colors (None: none): one [n_b,3] array per
         fragment, float in [0, 1] or uint8, carried to fo.colors through every stage (a voxel's colour is the mean of
         its points');
      1b. denoise (None: nothing, the chain and the result as without it): {"method": "statistical", "nb_neighbors":
         20, "std_ratio": 2.0} or {"method": "radius", "nb_points": 16, "radius": None} (options may be left out) —
         fo.statistical_outliers / fo.radius_outliers per fragment, then fo = fo.select(keep): every later stage,
         the fused scene included, sees the kept points only; or {"method": "cluster", "min_points": 10, "min_size":
         100, "eps": None} — fo.cluster_dbscan(eps, min_points) per fragment (eps None: the index's cell, at most
         it), fo.cluster_keep(min_size): the clusters of fewer than min_size points and the noise go, which removes
         the detached blobs the two outlier filters let through;
      2. estimate_normals(normal_radius, viewpoints) — viewpoints [n,3] in the fragments' own frames, None: their
         origins (where a range sensor stood);
      3. compute_fpfh(fpfh_radius);  4. lib.fpfh.register_fpfh on all pairs i < j with `seed` and
         checkers=ransac_checkers (True or a dict: RANSAC with correspondence checkers and 100000 draws), or with
         coarse="fgr" lib.fpfh.register_fgr (Fast Global Registration, `seed` keying its tuple filter; not with
         ransac_checkers.  It wants matches with tens of percent inliers: RANSAC stays the default);
         keypoints (None: every point is matched, as without it): True, or a dict of fo.iss_keypoints' options and
         "match" ('keypoints' or 'all', lib.fpfh.match_keypoints) — ISS keypoints are detected once and the matching
         of either estimator runs on them (not with init)
         (init [P,4,4], x_j ~ T x_i for the pairs i < j in that order, replaces 3 and 4);
      5. the overlap gate of the pairwise benchmark: a pair is kept when FragmentOverlap.ratios >= overlap_threshold
         (None: the benchmark's value for `dataset`, 0.3 for '3d_match', 0.23 for 'redwood');
      6. lib.icp.icp_refine (method 'point_to_point' / 'point_to_plane'), gicp_refine ('generalized') or
         colored_icp_refine ('colored': needs colors; fo.compute_color_gradients(normal_radius) runs after step 2,
         the share of the geometric term is icp_lambda_geometric) on the kept pairs; icp_kernel (None: every
         correspondence weighs 1, the chain and the result as without it): one of
         lib.icp.ROBUST_KERNELS with its scale icp_kernel_k, None: voxel_size, the sampling scale of the centroids
         (a documented default, not a tuned value; 'gm' takes a squared length, so give it one);  7. lib.icp.information_matrix;  8. synchronize(irls_iters=5);  9. optimize_pose_graph with the
         IRLS weights (line_process: with Open3D's line process and edge pruning, every kept pair an uncertain edge,
         preference_loop_closure, and the distance the information matrices used: icp_max_dist, None: the index's
         cell);  10. fuse_scene(voxel fuse_voxel, None: voxel_size) over the fragments connected to `anchor`.
    Returns a dict of R [n,3,3], t [n,3] and poses [n,4,4] (numpy fp64, fragment -> the anchor's frame), member [n],
    pairs: a dict of numpy arrays over the pairs i < j (pairs [P,2], T_coarse [P,4,4], overlap [P], kept bool [P],
    T [P,4,4] the refined estimate (the coarse one where the pair was not kept), fitness and rmse [P] of the
    refinement, 0 where not kept; with line_process also pruned bool [P]: the pose graph dropped the pair), sync and
    refined (the dicts of synchronize and optimize_pose_graph), fo, and scene (the dict of fuse_scene); with denoise
    also denoise: keep (numpy bool over the points of step 1, fo.parent_rows are the kept ones) and removed [n] (the
    points each fragment lost); with keypoints also keypoints: rows [K] (rows of fo.xyz, ascending) and off [n+1]
    (numpy int64)."""
    from lib.fpfh import register_fgr, register_fpfh
    from lib.icp import _check_kernel, colored_icp_refine, gicp_refine, icp_refine, information_matrix
    from lib.overlap import FragmentOverlap
    n = len(xyz_list)
    if coarse not in COARSE_METHODS:
        raise ValueError("register_scene: coarse must be one of %s, not %r" % (", ".join(COARSE_METHODS), coarse))
    if coarse == "fgr" and ransac_checkers is not False:
        raise ValueError("register_scene: ransac_checkers belongs to coarse='ransac', not to coarse='fgr'")
    pairs, init, viewpoints = _scene_arguments(n, voxel_size, method, dataset, init, viewpoints, colors,
                                               icp_lambda_geometric)
    if icp_kernel is not None and icp_kernel_k is None:
        icp_kernel_k = float(voxel_size)
    _check_kernel("register_scene", icp_kernel, icp_kernel_k)
    robust = {} if icp_kernel is None else {"kernel": icp_kernel, "kernel_k": icp_kernel_k}
    denoise = _denoise_arguments(denoise, 3.0 * float(voxel_size))
    keypoints = _keypoints_arguments(keypoints, 3.0 * float(voxel_size), init)
    threshold = OVERLAP_THRESHOLDS[dataset] if overlap_threshold is None else float(overlap_threshold)
    P = len(pairs)
    with_colors = {} if colors is None else {"colors": colors}
    if downsample:
        fo = FragmentOverlap(xyz_list, "FCGF", voxel_size, **with_colors)
    else:
        fo = FragmentOverlap(xyz_list, "3DMatch", radius=3.0 * float(voxel_size), **with_colors)
    denoised = None
    if denoise is not None:
        if denoise["method"] == "statistical":
            keep = fo.statistical_outliers(denoise["nb_neighbors"], denoise["std_ratio"])["keep"]
        elif denoise["method"] == "cluster":
            keep = fo.cluster_keep(fo.cluster_dbscan(denoise["eps"], denoise["min_points"]), denoise["min_size"])
        else:
            keep = fo.radius_outliers(denoise["nb_points"], denoise["radius"])["keep"]
        sizes = np.diff(fo.off)
        fo = fo.select(keep)
        denoised = {"keep": keep.cpu().numpy(), "removed": (sizes - np.diff(fo.off)).astype(np.int64)}
    fo.estimate_normals(normal_radius, viewpoints)
    if method == "colored":
        fo.compute_color_gradients(normal_radius)
    if init is None:
        fo.compute_fpfh(fpfh_radius)
        kp_args = {}
        if keypoints is not None:
            detected = fo.iss_keypoints(**{k: v for k, v in keypoints.items() if k != "match"})
            kp_args = {"keypoints": detected, "match": keypoints["match"]}
        if coarse == "fgr":
            T_coarse = np.asarray(register_fgr(fo, pairs, seed=seed, **kp_args)["T"], dtype=np.float64)
        else:
            T_coarse = np.asarray(register_fpfh(fo, pairs, seed=seed, checkers=ransac_checkers, **kp_args)["T"],
                                  dtype=np.float64)
    else:
        T_coarse = init
    overlap = fo.ratios(pairs, np.linalg.inv(T_coarse))      # the gate's `trans` is the inverse of the estimate
    kept = overlap >= threshold
    kp = pairs[kept]
    if method == "generalized":
        ref = gicp_refine(fo, kp, T_coarse[kept], max_dist=icp_max_dist, max_iters=icp_iters, epsilon=gicp_epsilon,
                          **robust)
    elif method == "colored":
        ref = colored_icp_refine(fo, kp, T_coarse[kept], max_dist=icp_max_dist, max_iters=icp_iters,
                                 lambda_geometric=icp_lambda_geometric, **robust)
    else:
        ref = icp_refine(fo, kp, T_coarse[kept], max_dist=icp_max_dist, max_iters=icp_iters, method=method, **robust)
    Tk = np.asarray(ref["T"], dtype=np.float64).reshape(-1, 4, 4)
    info = information_matrix(fo, kp, Tk, max_dist=icp_max_dist)
    sync = synchronize(Tk[:, :3, :3], Tk[:, :3, 3], kp, n, anchor=anchor, irls_iters=5)
    refined = optimize_pose_graph(np.asarray(sync["R"]), np.asarray(sync["t"]), Tk[:, :3, :3], Tk[:, :3, 3], kp,
                                  np.asarray(info["info"]), np.asarray(sync["weights"]), anchor=anchor,
                                  max_iters=refine_iters,
                                  **({} if not line_process else dict(
                                      line_process=True, preference_loop_closure=preference_loop_closure,
                                      max_correspondence_distance=float(fo.r if icp_max_dist is None
                                                                        else icp_max_dist))))
    R, t = np.asarray(refined["R"], dtype=np.float64), np.asarray(refined["t"], dtype=np.float64)
    member = np.asarray(refined["member"])
    scene = fuse_scene(fo, R, t, voxel_size if fuse_voxel is None else fuse_voxel, member=member,
                       min_frags=min_frags, min_points=min_points)
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, :3, :3], poses[:, :3, 3] = R, t
    T = T_coarse.copy()
    fitness, rmse = np.zeros(P), np.zeros(P)
    T[kept], fitness[kept], rmse[kept] = Tk, np.asarray(ref["fitness"]), np.asarray(ref["rmse"])
    records = {"pairs": pairs, "T_coarse": T_coarse, "overlap": overlap, "kept": kept, "T": T, "fitness": fitness,
               "rmse": rmse}
    if line_process:
        pruned = np.zeros(P, dtype=bool)
        pruned[kept] = ~np.asarray(refined["kept"], dtype=bool)
        records["pruned"] = pruned
    result = {"R": R, "t": t, "poses": poses, "member": member, "pairs": records, "sync": sync, "refined": refined,
              "fo": fo, "scene": scene}
    if denoised is not None:
        result["denoise"] = denoised
    if keypoints is not None:
        result["keypoints"] = {"rows": detected["rows"].cpu().numpy(), "off": detected["off"]}
    return result
