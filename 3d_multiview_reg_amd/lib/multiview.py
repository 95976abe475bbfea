"""Multiview stage: one globally consistent pose per fragment from a scene's pairwise estimates.

`synchronize` is the transformation synchronisation of the paper's sections 3.2-3.3 (closed-form weighted solve:
an eigenproblem for the rotations, a linear solve for the translations) with optional IRLS, on the GPU
(csrc/sync.hip mvr_sync_poses; the maths and the conventions are in DESIGN.md 4.18).  The
reference never released this stage, so there is no reference module behind this file.

Conventions: edge k = (i, j) with x_j ~ R_k x_i + t_k (source i, target j: lib.utils.pair_index order, the rot_est /
trans_est of filter_correspondences); pose (R_i, t_i) maps fragment i into the anchor's frame, X = R_i x_i + t_i.
"""
import torch

from lib import _native as N

STATUS_NOT_CONNECTED, STATUS_ITERATION_CAP, STATUS_EDGE_IGNORED = 1, 2, 4
MAX_FRAGS = 128   # include/mvreg.h MVR_SYNC_MAX_FRAGS


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else None


def synchronize(R_pair, t_pair, pairs, n_frags, weights=None, anchor=0, irls_iters=0, c_rot=0.1, c_trans=0.1,
                n_edges=None):
    """Poses of every fragment from pairwise estimates (batched over scenes, one launch).

    One scene: R_pair [E,3,3], t_pair [E,3] (or [E,3,1]), pairs [E,2], n_frags int, weights [E] or None (all ones).
    A batch: lists of such per-scene arrays with n_frags a list, or padded R_pair [S,E,3,3], t_pair [S,E,3],
    pairs [S,E,2], weights [S,E] with n_frags [S] and n_edges [S] (default E for every scene).
    Inputs are torch tensors or numpy arrays, fp32 or fp64; the solve is fp64.
    Returns a dict of fp64 R [N,3,3], t [N,3], int32 member [N], fp64 weights / res_rot / res_trans [E] (the last
    IRLS pass's weights and per-edge residuals) and int32 status (bits: 1 some fragment is not connected to the
    anchor and came out as identity with member 0, 2 an eigen-solve hit its iteration cap, 4 an edge was ignored or
    the scene is invalid); a batch adds a leading [S] (padded to the largest N and E).  The outputs stay on the
    device when R_pair was on the device; otherwise they come back on the host (numpy for numpy inputs)."""
    N.require_hip()
    was_numpy = not torch.is_tensor(R_pair if _as_list(R_pair) is None else R_pair[0])
    first = torch.as_tensor(R_pair if _as_list(R_pair) is None else R_pair[0])
    on_dev = first.device.type == "cuda"
    dev = first.device if on_dev else torch.device("cuda", torch.cuda.current_device())

    def f64(x, tail):
        return torch.as_tensor(x).to(dev, torch.float64).reshape((-1,) + tail)

    lists = _as_list(R_pair)
    if lists is not None:   # per-scene lists -> padded
        S = len(lists)
        nf = [int(v) for v in n_frags]
        if not (len(t_pair) == len(pairs) == len(nf) == S) or (weights is not None and len(weights) != S):
            raise ValueError("synchronize: the per-scene lists must have one entry per scene")
        Rs = [f64(x, (3, 3)) for x in R_pair]
        ne = [int(x.shape[0]) for x in Rs]
        Emax = max(ne) if ne else 0
        Rp = torch.zeros(S, Emax, 3, 3, dtype=torch.float64, device=dev)
        tp = torch.zeros(S, Emax, 3, dtype=torch.float64, device=dev)
        ij = torch.zeros(S, Emax, 2, dtype=torch.int32, device=dev)
        w = None if weights is None else torch.zeros(S, Emax, dtype=torch.float64, device=dev)
        for s in range(S):
            Rp[s, :ne[s]] = Rs[s]
            tp[s, :ne[s]] = f64(t_pair[s], (3,))
            ij[s, :ne[s]] = torch.as_tensor(pairs[s]).to(dev, torch.int32).reshape(-1, 2)
            if w is not None:
                w[s, :ne[s]] = f64(weights[s], ())
        batched = True
    else:
        Rp = torch.as_tensor(R_pair).to(dev, torch.float64)
        batched = Rp.dim() == 4
        if Rp.dim() not in (3, 4) or tuple(Rp.shape[-2:]) != (3, 3):
            raise ValueError("synchronize: R_pair must be [E,3,3] or [S,E,3,3]")
        if not batched:
            Rp = Rp.unsqueeze(0)
        S, Emax = Rp.shape[0], Rp.shape[1]
        Rp = Rp.contiguous()
        tp = torch.as_tensor(t_pair).to(dev, torch.float64).reshape(S, Emax, 3).contiguous()
        ij = torch.as_tensor(pairs).to(dev, torch.int32).reshape(S, Emax, 2).contiguous()
        w = None if weights is None else torch.as_tensor(weights).to(dev, torch.float64).reshape(S, Emax).contiguous()
        nf = [int(v) for v in torch.as_tensor(n_frags).reshape(-1).tolist()]
        if len(nf) != S:
            raise ValueError("synchronize: n_frags must give one count per scene")
        ne = [Emax] * S if n_edges is None else [int(v) for v in torch.as_tensor(n_edges).reshape(-1).tolist()]
        if len(ne) != S or min(ne + [0]) < 0 or max(ne + [0]) > Emax:
            raise ValueError("synchronize: n_edges must be [S] with 0 <= n_edges <= E")
    Fmax = max(nf + [0])
    if min(nf + [0]) < 0 or Fmax > MAX_FRAGS:
        raise ValueError("synchronize: n_frags must be within [0, %d]" % MAX_FRAGS)
    if not 0 <= int(anchor) < max(Fmax, 1):
        raise ValueError("synchronize: anchor outside the fragments")
    n_e = torch.tensor(ne, dtype=torch.int32).to(dev)
    n_f = torch.tensor(nf, dtype=torch.int32).to(dev)
    R = torch.empty(S, Fmax, 3, 3, dtype=torch.float64, device=dev)
    t = torch.empty(S, Fmax, 3, dtype=torch.float64, device=dev)
    member = torch.zeros(S, Fmax, dtype=torch.int32, device=dev)
    w_out, res_rot, res_trans = (torch.zeros(S, Emax, dtype=torch.float64, device=dev) for _ in range(3))
    status = torch.zeros(S, dtype=torch.int32, device=dev)
    if S and Fmax:
        R[:] = torch.eye(3, dtype=torch.float64, device=dev)   # the rows past a scene's n_frags: identity as well
        t.zero_()
        L = N.lib()
        ws = N.workspace(L.mvr_sync_workspace_bytes(S, Fmax, Emax), dev)
        N.check(L.mvr_sync_poses(N.ptr(Rp), N.ptr(tp), N.ptr(ij), N.ptr(w), Emax, N.ptr(n_e), N.ptr(n_f), S, Fmax,
                                 Emax, int(anchor), int(irls_iters), float(c_rot), float(c_trans), N.ptr(R), N.ptr(t),
                                 Fmax, N.ptr(member), N.ptr(w_out), N.ptr(res_rot), N.ptr(res_trans), N.ptr(status),
                                 N.ptr(ws), ws.numel(), N.stream()), "mvr_sync_poses")
    out = {"R": R, "t": t, "member": member, "weights": w_out, "res_rot": res_rot, "res_trans": res_trans,
           "status": status}
    if not batched:
        out = {k: v[0] for k, v in out.items()}
    if not on_dev:
        out = {k: v.cpu() for k, v in out.items()}
        if was_numpy:
            out = {k: v.numpy() for k, v in out.items()}
    return out


PG_STATUS_NOT_CONNECTED, PG_STATUS_ITERATION_CAP, PG_STATUS_EDGE_IGNORED, PG_STATUS_FACTORISATION = 1, 2, 4, 8


def optimize_pose_graph(R, t, R_pair, t_pair, pairs, info, weights=None, anchor=0, max_iters=20, lambda0=1e-6,
                        tol_cost=1e-9, tol_step=1e-10, return_trace=False, n_frags=None, n_edges=None):
    """Refine poses jointly over SE(3) with per-edge information matrices (batched over scenes, one launch;
    csrc/posegraph.hip mvr_posegraph_optimize): Levenberg-Marquardt on sum_k w_k xi_k^T info_k xi_k,
    xi_k = (v, omega) of M_j^-1 M_i T_k^-1, from the poses `synchronize` returns, the anchor held.  The stage of
    Open3D's global_optimization; Open3D parity is unpinned, there is no line process or robust kernel.

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
    device; otherwise they come back on the host (numpy for numpy inputs)."""
    if int(max_iters) < 0:
        raise ValueError("optimize_pose_graph: max_iters must not be negative")
    if not (float(lambda0) >= 0.0 and float(lambda0) < float("inf")):
        raise ValueError("optimize_pose_graph: lambda0 must be finite and not negative")
    if not (tol_cost >= 0.0 and tol_step >= 0.0):
        raise ValueError("optimize_pose_graph: the tolerances must not be negative")
    lists = _as_list(R)
    first = R if lists is None else (R[0] if len(R) else torch.zeros(0, 3, 3))
    was_numpy = not torch.is_tensor(first)
    first = torch.as_tensor(first)
    on_dev = first.device.type == "cuda"
    if on_dev:
        dev = first.device
    elif torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        dev = torch.device("cpu")   # the shapes are still checked; require_hip() below then raises

    def f64(x, tail):
        return torch.as_tensor(x).to(dev, torch.float64).reshape((-1,) + tail)

    if lists is not None:   # per-scene lists -> padded
        S = len(lists)
        others = (t, R_pair, t_pair, pairs, info) + (() if weights is None else (weights,))
        if any(_as_list(x) is None or len(x) != S for x in others):
            raise ValueError("optimize_pose_graph: the per-scene lists must have one entry per scene")
        R0s = [f64(x, (3, 3)) for x in R]
        Rs = [f64(x, (3, 3)) for x in R_pair]
        nf, ne = [int(x.shape[0]) for x in R0s], [int(x.shape[0]) for x in Rs]
        Fmax, Emax = max(nf + [0]), max(ne + [0])
        R0 = torch.zeros(S, Fmax, 3, 3, dtype=torch.float64, device=dev)
        t0 = torch.zeros(S, Fmax, 3, dtype=torch.float64, device=dev)
        Rp = torch.zeros(S, Emax, 3, 3, dtype=torch.float64, device=dev)
        tp = torch.zeros(S, Emax, 3, dtype=torch.float64, device=dev)
        ij = torch.zeros(S, Emax, 2, dtype=torch.int32, device=dev)
        lam = torch.zeros(S, Emax, 36, dtype=torch.float64, device=dev)
        w = None if weights is None else torch.zeros(S, Emax, dtype=torch.float64, device=dev)
        for s in range(S):
            ts, tps, ijs, ls = f64(t[s], (3,)), f64(t_pair[s], (3,)), torch.as_tensor(pairs[s]).reshape(-1, 2), \
                f64(info[s], (36,))
            if ts.shape[0] != nf[s] or not (tps.shape[0] == ijs.shape[0] == ls.shape[0] == ne[s]):
                raise ValueError("optimize_pose_graph: scene %d: one t per pose and one t_pair, pair and info per "
                                 "edge" % s)
            R0[s, :nf[s]], t0[s, :nf[s]] = R0s[s], ts
            Rp[s, :ne[s]], tp[s, :ne[s]], lam[s, :ne[s]] = Rs[s], tps, ls
            ij[s, :ne[s]] = ijs.to(dev, torch.int32)
            if w is not None:
                ws_ = f64(weights[s], ())
                if ws_.shape[0] != ne[s]:
                    raise ValueError("optimize_pose_graph: scene %d: one weight per edge" % s)
                w[s, :ne[s]] = ws_
        batched = True
    else:
        R0 = torch.as_tensor(R).to(dev, torch.float64)
        Rp = torch.as_tensor(R_pair).to(dev, torch.float64)
        if R0.dim() not in (3, 4) or tuple(R0.shape[-2:]) != (3, 3):
            raise ValueError("optimize_pose_graph: R must be [N,3,3] or [S,F,3,3]")
        batched = R0.dim() == 4
        if Rp.dim() != R0.dim() or tuple(Rp.shape[-2:]) != (3, 3):
            raise ValueError("optimize_pose_graph: R_pair must be [E,3,3] or [S,E,3,3], as R is")
        if not batched:
            R0, Rp = R0.unsqueeze(0), Rp.unsqueeze(0)
        if Rp.shape[0] != R0.shape[0]:
            raise ValueError("optimize_pose_graph: R and R_pair must hold the same scenes")
        S, Fmax, Emax = R0.shape[0], R0.shape[1], Rp.shape[1]
        R0, Rp = R0.contiguous(), Rp.contiguous()
        try:
            t0 = torch.as_tensor(t).to(dev, torch.float64).reshape(S, Fmax, 3).contiguous()
            tp = torch.as_tensor(t_pair).to(dev, torch.float64).reshape(S, Emax, 3).contiguous()
            ij = torch.as_tensor(pairs).to(dev, torch.int32).reshape(S, Emax, 2).contiguous()
            lam = torch.as_tensor(info).to(dev, torch.float64).reshape(S, Emax, 36).contiguous()
            w = None if weights is None else \
                torch.as_tensor(weights).to(dev, torch.float64).reshape(S, Emax).contiguous()
        except RuntimeError:
            raise ValueError("optimize_pose_graph: t must hold one row per pose; t_pair, pairs, info and weights "
                             "one per edge") from None
        nf = [Fmax] * S if n_frags is None else [int(v) for v in torch.as_tensor(n_frags).reshape(-1).tolist()]
        ne = [Emax] * S if n_edges is None else [int(v) for v in torch.as_tensor(n_edges).reshape(-1).tolist()]
        if len(nf) != S or min(nf + [0]) < 0 or max(nf + [0]) > Fmax:
            raise ValueError("optimize_pose_graph: n_frags must be [S] with 0 <= n_frags <= F")
        if len(ne) != S or min(ne + [0]) < 0 or max(ne + [0]) > Emax:
            raise ValueError("optimize_pose_graph: n_edges must be [S] with 0 <= n_edges <= E")
    if Fmax > MAX_FRAGS:
        raise ValueError("optimize_pose_graph: at most %d fragments per scene" % MAX_FRAGS)
    if not 0 <= int(anchor) < max(Fmax, 1):
        raise ValueError("optimize_pose_graph: anchor outside the fragments")
    N.require_hip()
    rows = int(max_iters) + 1
    n_e = torch.tensor(ne, dtype=torch.int32).to(dev)
    n_f = torch.tensor(nf, dtype=torch.int32).to(dev)
    Ro, to = R0.clone(), t0.clone()      # the rows past a scene's n_frags keep their input
    member = torch.zeros(S, Fmax, dtype=torch.int32, device=dev)
    cost = torch.zeros(S, 2, dtype=torch.float64, device=dev)
    iters, status = (torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2))
    trace = torch.full((S, rows), -1.0, dtype=torch.float64, device=dev) if return_trace else None
    if S and Fmax:
        L = N.lib()
        ws = N.workspace(L.mvr_posegraph_workspace_bytes(S, Fmax, Emax), dev)
        N.check(L.mvr_posegraph_optimize(N.ptr(Rp), N.ptr(tp), N.ptr(ij), N.ptr(w), N.ptr(lam), Emax, N.ptr(n_e),
                                         N.ptr(n_f), S, Fmax, Emax, int(anchor), N.ptr(R0), N.ptr(t0),
                                         int(max_iters), float(lambda0), float(tol_cost), float(tol_step), N.ptr(Ro),
                                         N.ptr(to), Fmax, N.ptr(member), N.ptr(cost), N.ptr(iters), N.ptr(status),
                                         N.ptr(trace), N.ptr(ws), ws.numel(), N.stream()), "mvr_posegraph_optimize")
    out = {"R": Ro, "t": to, "member": member, "cost": cost, "iters": iters, "status": status}
    if return_trace:
        out["trace"] = trace
    if not batched:
        out = {k: v[0] for k, v in out.items()}
    if not on_dev:
        out = {k: v.cpu() for k, v in out.items()}
        if was_numpy:
            out = {k: v.numpy() for k, v in out.items()}
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
