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
