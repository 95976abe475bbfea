"""numpy restatement of the pose-graph refinement (csrc/posegraph.hip mvr_posegraph_optimize; DESIGN.md 4.22,
include/mvreg.h).  This file is the normative text of the loop.

Conventions: pose M_i: X = R_i x_i + t_i; edge k = (i, j): x_j ~ T_k x_i; the anchor's pose is held.

    residual   D_k = M_j^-1 M_i T_k^-1,  xi_k = (v, omega): v the translation of D_k, omega = log of its rotation
               (a = vee(D - D^T) / 2, theta = atan2(|a|, (tr D - 1) / 2), omega = a theta / |a|)
    cost       c = sum_k w_k xi_k^T L_k xi_k,  L_k = (info_k + info_k^T) / 2
    update     delta_i = (dv, dw), on the left: R_i <- Exp(dw) R_i, t_i <- Exp(dw) t_i + dv
    Jacobian   first order: d xi_k / d delta_i = A_k, d xi_k / d delta_j = -A_k,
               A_k = Ad(M_j^-1) = [[R_j^T, -R_j^T [t_j]x], [0, R_j^T]]
    H, g       H = sum w J^T L J, g = sum w J^T L xi; rows and columns of the anchor and of non-members -> identity
    members    reachable from the anchor over valid edges with w > 0; an edge with a non-member end gets weight 0
    loop       lam = lambda0; converged = (c == 0)
               while not converged and trials < max_iters:
                   solve (H + lam diag H) delta = -g        (Cholesky; a pivot <= 0: a rejected trial, lam *= 10,
                                                             no candidate, no step test)
                   candidate poses, c'
                   c' < c: accept, lam /= 10, converged if c - c' <= tol_cost c      else: lam *= 10
                   converged if max|delta| <= tol_step; converged if c == 0
               status 2: trials == max_iters, not converged, a tolerance positive
               status 8: the last trial's factorisation failed
    ignored    an edge with an index out of range, i == j, non-finite T / info / w, w < 0, or
               max|info - info^T| > 1e-9 |info|_F: status 4, weight 0
    invalid    anchor >= n_frags or a non-finite initial pose: poses copied through, member 0, status 4 | 1

Every trial reports its margins, so a test can assert that no accept / reject or stop decision was made by rounding:
accept = (c - c') / c, and per stop test the distance of its quantity from its threshold.
"""
import functools

import numpy as np


def skew(y):
    return np.array([[0.0, -y[2], y[1]], [y[2], 0.0, -y[0]], [-y[1], y[0], 0.0]])


def so3_log(R):
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt(a @ a)
    th = np.arctan2(s, 0.5 * (np.trace(R) - 1.0))
    return a * (th / s if s > 1e-8 else 1.0 + th * th / 6.0)


def so3_exp(w):
    t2 = float(w @ w)
    th = np.sqrt(t2)
    A = np.sin(th) / th if th > 1e-8 else 1.0 - t2 / 6.0
    B = (1.0 - np.cos(th)) / t2 if th > 1e-8 else 0.5 - t2 / 24.0
    K = skew(w)
    return np.eye(3) + A * K + B * (K @ K)


def residual(Ri, ti, Rj, tj, Rk, tk):
    P = Ri @ Rk.T
    return np.concatenate([Rj.T @ (ti - P @ tk - tj), so3_log(Rj.T @ P)])


def adjoint(Rj, tj):
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = Rj.T
    A[:3, 3:] = -Rj.T @ skew(tj)
    return A


def edge_weights(n, anchor, Rp, tp, ij, w, info):
    """-> (the weight of every edge that counts, member [n], ignored any)"""
    E = len(ij)
    w0 = np.full(E, -1.0)
    for e in range(E):
        i, j = int(ij[e, 0]), int(ij[e, 1])
        L = info[e]
        ok = 0 <= i < n and 0 <= j < n and i != j and np.isfinite(w[e]) and w[e] >= 0
        ok = ok and np.all(np.isfinite(Rp[e])) and np.all(np.isfinite(tp[e])) and np.all(np.isfinite(L))
        ok = ok and not np.max(np.abs(L - L.T)) > 1e-9 * np.sqrt(np.sum(L * L))
        if ok:
            w0[e] = w[e]
    member = np.zeros(n, np.int32)
    member[anchor] = 1
    changed = True
    while changed:
        changed = False
        for e in range(E):
            if w0[e] > 0 and member[ij[e, 0]] != member[ij[e, 1]]:
                member[ij[e, 0]] = member[ij[e, 1]] = 1
                changed = True
    wc = np.maximum(w0, 0.0)
    for e in range(E):
        if wc[e] > 0 and not member[ij[e, 0]]:
            wc[e] = 0.0
    return wc, member, bool(np.any(w0 < 0))


def cost(R, t, Rp, tp, ij, wc, L):
    c = 0.0
    for e in np.nonzero(wc > 0)[0]:
        i, j = ij[e]
        xi = residual(R[i], t[i], R[j], t[j], Rp[e], tp[e])
        c += wc[e] * (xi @ L[e] @ xi)
    return c


def cost_evaluation_floor(sc, R, t, anchor=0, seeds=(0, 1, 2)):
    """How far the cost of one set of poses moves when the same sum is evaluated another way: the edges in a
    shuffled order, each term as xi . (w L xi) instead of w ((xi L) xi), and the residual's products associated the
    other way round, D = (R_j^T R_i) R_k^T and v = R_j^T (t_i - t_j) - D t_k -> the largest |difference| over
    `seeds`.  What a second implementation of the evaluation (the kernel's: another edge order, fused multiply-adds)
    is expected to differ by; the cholesky / solve pair of runs cannot show it, they share the evaluation."""
    R, t, Rp, tp, ij, w, info = _arrays(R, t, sc["R_pair"], sc["t_pair"], sc["ij"], sc["w"], sc["info"])
    wc, _, _ = edge_weights(len(R), anchor, Rp, tp, ij, w, info)
    L = np.nan_to_num(0.5 * (info + np.transpose(info, (0, 2, 1))))
    ref = cost(R, t, Rp, tp, ij, wc, L)
    worst = 0.0
    live = np.nonzero(wc > 0)[0]
    for seed in seeds:
        c = 0.0
        for e in np.random.default_rng(seed).permutation(live):
            i, j = ij[e]
            D = (R[j].T @ R[i]) @ Rp[e].T
            xi = np.concatenate([R[j].T @ (t[i] - t[j]) - D @ tp[e], so3_log(D)])
            c += xi @ ((wc[e] * L[e]) @ xi)
        worst = max(worst, abs(c - ref))
    return worst


def system(R, t, Rp, tp, ij, wc, L, member, anchor):
    """-> H [6n,6n], g [6n] with the identity rows and columns in place"""
    n = len(R)
    H, g = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    solved = member.astype(bool).copy()
    solved[anchor] = False
    for e in np.nonzero(wc > 0)[0]:
        i, j = int(ij[e, 0]), int(ij[e, 1])
        xi = residual(R[i], t[i], R[j], t[j], Rp[e], tp[e])
        A = adjoint(R[j], t[j])
        B = wc[e] * (A.T @ L[e] @ A)
        b = wc[e] * (A.T @ (L[e] @ xi))
        si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
        if solved[i]:
            H[si, si] += B
            g[si] += b
        if solved[j]:
            H[sj, sj] += B
            g[sj] -= b
        if solved[i] and solved[j]:
            H[si, sj] -= B
            H[sj, si] -= B
    for f in np.nonzero(~solved)[0]:
        H[6 * f:6 * f + 6, 6 * f:6 * f + 6] = np.eye(6)
    return H, g


def gradient_norm(R, t, Rp, tp, ij, w, info, anchor=0):
    """|g| at the poses (R, t) over the solved fragments"""
    R, t, Rp, tp, ij, w, info = _arrays(R, t, Rp, tp, ij, w, info)
    wc, member, _ = edge_weights(len(R), anchor, Rp, tp, ij, w, info)
    L = 0.5 * (info + np.transpose(info, (0, 2, 1)))
    return float(np.linalg.norm(system(R, t, Rp, tp, ij, wc, np.nan_to_num(L), member, anchor)[1]))


def _arrays(R, t, Rp, tp, ij, w, info):
    R = np.array(R, np.float64).reshape(-1, 3, 3)
    E = np.asarray(Rp).reshape(-1, 3, 3).shape[0]
    return (R, np.array(t, np.float64).reshape(-1, 3), np.asarray(Rp, np.float64).reshape(-1, 3, 3),
            np.asarray(tp, np.float64).reshape(-1, 3), np.asarray(ij).reshape(-1, 2).astype(np.int64),
            np.ones(E) if w is None else np.asarray(w, np.float64).reshape(-1),
            np.asarray(info, np.float64).reshape(-1, 6, 6))


def optimize(R0, t0, Rp, tp, ij, info, w=None, anchor=0, max_iters=20, lambda0=1e-6, tol_cost=1e-9, tol_step=1e-10,
             solver="cholesky"):
    """One scene.  solver 'cholesky': np.linalg.cholesky and two triangular solves; 'solve': np.linalg.solve (after
    the same positive-definiteness test).  -> dict(R, t, member, cost (initial, final), iters, status,
    trace [max_iters + 1], accepted [bool per trial], failed [bool per trial], steps [max|delta| per trial],
    margins [(accept margin |c - c'| / c or inf, stop margin or inf) per trial])"""
    R, t, Rp, tp, ij, w, info = _arrays(R0, t0, Rp, tp, ij, w, info)
    n = len(R)
    trace = np.full(max_iters + 1, -1.0)
    out = {"R": R, "t": t, "member": np.zeros(n, np.int32), "cost": np.zeros(2), "iters": 0, "status": 0,
           "trace": trace, "accepted": [], "failed": [], "margins": [], "steps": []}
    if n == 0:
        out["status"] = 4 if len(ij) else 0
        return out
    if anchor >= n or not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        out["status"] = 4 | 1
        return out
    wc, member, ignored = edge_weights(n, anchor, Rp, tp, ij, w, info)
    status = (4 if ignored else 0) | (1 if member.sum() < n else 0)
    L = np.nan_to_num(0.5 * (info + np.transpose(info, (0, 2, 1))))   # ignored edges' NaNs never count
    c = cost(R, t, Rp, tp, ij, wc, L)
    c_init = c
    trace[0] = c
    lam, k, converged, failed = lambda0, 0, c == 0.0, False
    while not converged and k < max_iters:
        H, g = system(R, t, Rp, tp, ij, wc, L, member, anchor)
        M = H + lam * np.diag(np.diag(H))
        for f in range(n):   # the identity rows stay identity
            if not member[f] or f == anchor:
                M[6 * f:6 * f + 6, 6 * f:6 * f + 6] = np.eye(6)
        k += 1
        try:
            if not np.all(np.isfinite(M)):
                raise np.linalg.LinAlgError
            C = np.linalg.cholesky(M)
            failed = False
        except np.linalg.LinAlgError:
            failed = True
        if failed:
            lam *= 10.0
            out["accepted"].append(False)
            out["failed"].append(True)
            out["margins"].append((np.inf, np.inf))
            out["steps"].append(np.nan)
            trace[k] = c
            continue
        if solver == "cholesky":
            delta = -np.linalg.solve(C.T, np.linalg.solve(C, g))
        else:
            delta = -np.linalg.solve(M, g)
        Rc, tc = R.copy(), t.copy()
        for f in range(n):
            Ex = so3_exp(delta[6 * f + 3:6 * f + 6])
            Rc[f] = Ex @ R[f]
            tc[f] = Ex @ t[f] + delta[6 * f:6 * f + 3]
        cn = cost(Rc, tc, Rp, tp, ij, wc, L)
        step = float(np.max(np.abs(delta)))
        accepted = cn < c
        m_accept = abs(c - cn) / c
        stops = [abs(step - tol_step) / max(tol_step, 1e-300)] if tol_step > 0 else []
        if accepted:
            if tol_cost > 0:
                stops.append(abs((c - cn) - tol_cost * c) / (tol_cost * c))
            if c - cn <= tol_cost * c:
                converged = True
            R, t, c = Rc, tc, cn
            lam /= 10.0
        else:
            lam *= 10.0
        if step <= tol_step:
            converged = True
        if c == 0.0:
            converged = True
        out["accepted"].append(bool(accepted))
        out["failed"].append(False)
        out["margins"].append((m_accept, min(stops + [np.inf])))
        out["steps"].append(step)
        trace[k] = c
    if not converged and k == max_iters and (tol_cost > 0 or tol_step > 0):
        status |= 2
    if failed:
        status |= 8
    out.update(R=R, t=t, member=member, cost=np.array([c_init, c]), iters=k, status=status)
    return out


# --------------------------------------------------------------------------------------------------- the test scenes
def random_rotation(rng, deg=None):
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    th = rng.uniform(0, np.pi) if deg is None else np.deg2rad(deg)
    return so3_exp(a * th)


def scene(n, seed, edges="all", noise=False, zero_weights=0, n_points=40, start=(3.0, 0.05)):
    """A seeded scene: n fragments of random poses (fragment 0 at the identity), edges 'all' (every i < j) or 'ring'
    (a ring plus n // 2 chords), T_k exact or (noise) perturbed by 1 degree / 1 cm, info_k from the information oracle
    on n_points random points per edge, weights in [0.5, 1.5] of which `zero_weights` chords are 0, and initial poses
    off by start = (degrees, metres) (the anchor exact).
    -> dict(R_gt, t_gt, R0, t0, R_pair, t_pair, ij, info, w)"""
    import info_oracle
    rng = np.random.default_rng(seed)
    Rg = np.stack([np.eye(3)] + [random_rotation(rng) for _ in range(n - 1)])
    tg = np.concatenate([np.zeros((1, 3)), rng.uniform(-2, 2, (n - 1, 3))])
    if edges == "all":
        ij = [(i, j) for i in range(n) for j in range(i + 1, n)]
        chords = list(range(len(ij)))
    else:
        ij = [(i, (i + 1) % n) for i in range(n)] if n > 2 else [(0, 1)][:n - 1]
        n_ring = len(ij)
        for _ in range(n // 2):
            i, j = rng.choice(n, 2, replace=False)
            ij.append((int(i), int(j)))
        chords = list(range(n_ring, len(ij)))
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    E = len(ij)
    Rp, tp, info = np.zeros((E, 3, 3)), np.zeros((E, 3)), np.zeros((E, 6, 6))
    for e, (i, j) in enumerate(ij):
        Rk = Rg[j].T @ Rg[i]
        tk = Rg[j].T @ (tg[i] - tg[j])
        if noise:
            D = random_rotation(rng, 1.0)
            u = rng.standard_normal(3)
            Rk, tk = D @ Rk, D @ tk + 0.01 * u / np.linalg.norm(u)
        Rp[e], tp[e] = Rk, tk
        info[e] = info_oracle.information_from_points(rng.uniform(-1.5, 1.5, (n_points, 3)))
    w = rng.uniform(0.5, 1.5, E)
    if zero_weights:
        w[rng.choice(chords, min(zero_weights, len(chords)), replace=False)] = 0.0
    R0, t0 = Rg.copy(), tg.copy()
    for f in range(1, n):
        u = rng.standard_normal(3)
        R0[f] = random_rotation(rng, start[0]) @ Rg[f]
        t0[f] = tg[f] + start[1] * u / np.linalg.norm(u)
    return {"R_gt": Rg, "t_gt": tg, "R0": R0, "t0": t0, "R_pair": Rp, "t_pair": tp, "ij": ij, "info": info, "w": w}


def run(sc, **kw):
    return optimize(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"], **kw)


def pose_error(R, t, Rg, tg):
    """(largest rotation angle in radians, largest translation distance) between two pose sets"""
    ang = [np.linalg.norm(so3_log(a.T @ b)) for a, b in zip(R, Rg)]
    return float(max(ang + [0.0])), float(np.max(np.linalg.norm(np.asarray(t) - np.asarray(tg), axis=1), initial=0.0))


def truncated(sc, E):
    """the scene with its first E edges"""
    out = dict(sc)
    for k in ("R_pair", "t_pair", "ij", "info", "w"):
        out[k] = sc[k][:E].copy()
    return out


def with_bad_edges(sc):
    """the scene plus a repeated edge, an edge given as (j, i), and every kind of edge that is ignored; one existing
    edge gets w = 0"""
    n = len(sc["R0"])
    rng = np.random.default_rng(99)
    Rp, tp, ij, info, w = (list(sc[k]) for k in ("R_pair", "t_pair", "ij", "info", "w"))
    w[2] = 0.0

    def add(e, i=None, j=None, wgt=1.0, R=None, t=None, L=None):
        Rp.append(sc["R_pair"][e].copy() if R is None else R)
        tp.append(sc["t_pair"][e].copy() if t is None else t)
        ij.append((sc["ij"][e][0] if i is None else i, sc["ij"][e][1] if j is None else j))
        info.append(sc["info"][e].copy() if L is None else L)
        w.append(wgt)

    nan = np.nan
    add(3)                                                                   # repeated
    i5, j5 = sc["ij"][5]
    add(5, i=j5, j=i5, R=sc["R_pair"][5].T, t=-sc["R_pair"][5].T @ sc["t_pair"][5])   # (j, i) with the inverse
    add(0, i=4, j=4)                                                         # i == j
    add(0, i=-1)
    add(0, j=n)
    add(1, R=sc["R_pair"][1] * np.where(np.arange(9).reshape(3, 3) == 4, nan, 1.0))
    add(1, t=np.array([0.0, np.inf, 0.0]))
    L = sc["info"][6].copy()
    L[2, 5] = nan
    add(6, L=L)
    add(7, wgt=nan)
    add(7, wgt=-0.5)
    add(7, wgt=np.inf)
    L = sc["info"][8].copy()
    L[1, 4] += 1e-8 * np.linalg.norm(L)
    add(8, L=L)                                                              # not symmetric to 1e-9 of its norm
    L = sc["info"][9].copy()
    L[1, 4] += 1e-11 * np.linalg.norm(L)
    add(9, L=L, wgt=float(rng.uniform(0.5, 1.5)))                            # symmetric enough: counts, symmetrised
    out = dict(sc)
    out.update(R_pair=np.asarray(Rp), t_pair=np.asarray(tp), ij=np.asarray(ij, np.int64), info=np.asarray(info),
               w=np.asarray(w))
    return out


N_IGNORED = 10      # of with_bad_edges


def disconnected(seed=1):
    """9 fragments: 0..5 all pairs, 6..8 all pairs among themselves, nothing between"""
    sc = scene(9, seed, "all", True, 0)
    keep = [e for e, (i, j) in enumerate(sc["ij"]) if (i < 6) == (j < 6)]
    out = dict(sc)
    for k in ("R_pair", "t_pair", "ij", "info", "w"):
        out[k] = sc[k][keep]
    return out


def zero_info(only_edge, seed=1):
    """a scene of 6 with one all-zero information matrix: on one edge of many (all pairs), or on the only edge that
    reaches fragment 3 (ring; its other edges removed), which leaves that fragment's diagonal block of H zero"""
    if not only_edge:
        sc = scene(6, seed, "all", True, 0)
        sc["info"][4] = 0.0
        return sc
    sc = scene(6, seed, "ring", True, 0)
    keep = [e for e, (i, j) in enumerate(sc["ij"]) if 3 not in (i, j) or (i, j) == (2, 3)]
    for k in ("R_pair", "t_pair", "ij", "info", "w"):
        sc[k] = sc[k][keep]
    e23 = [e for e, (i, j) in enumerate(sc["ij"]) if (i, j) == (2, 3)]
    assert len(e23) == 1 and sum(3 in (i, j) for i, j in sc["ij"]) == 1
    sc["info"][e23[0]] = 0.0
    return sc


def cut_by_bad_edge(seed=1):
    """3 fragments on the chain (0,1), (1,2) whose second edge has a NaN in its rotation, plus a self-loop (2,2): the
    ignored edge is the only way to fragment 2, so the edge test decides the component"""
    sc = scene(3, seed, "all", True, 0)
    keep = [e for e, (i, j) in enumerate(sc["ij"]) if (i, j) in ((0, 1), (1, 2))]
    assert len(keep) == 2
    for k in ("R_pair", "t_pair", "ij", "info", "w"):
        sc[k] = np.concatenate([sc[k][keep], sc[k][keep[1:]]])
    sc["R_pair"][1, 0, 2] = np.nan
    sc["ij"][2] = (2, 2)
    return sc


def n1_bad_edges():
    """1 fragment with two edges that cannot count, (0,0) and (0,1), unit weights: nothing to optimise, status 4"""
    sc = scene(1, 1)
    sc.update(R_pair=np.tile(np.eye(3), (2, 1, 1)), t_pair=np.zeros((2, 3)), ij=np.array([[0, 0], [0, 1]], np.int64),
              info=np.tile(np.eye(6), (2, 1, 1)), w=np.ones(2))
    return sc


EDGE_COUNTS = (0, 1, 127, 128, 129, 255, 256, 257)    # the kernel stages the edges' endpoints in chunks of 256
TWO = dict(max_iters=2, tol_cost=0.0, tol_step=0.0)
STEP = dict(tol_cost=0.0, tol_step=1e-4)     # exact edges: the third trial's step is 3e-10 .. 2e-5, the second's > 1e-3


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (scene, keyword arguments of optimize): every scene of test_gpu_posegraph.py, all from seed 1.  The
    noisy scenes run a fixed number of trials (both tolerances 0) or stop on a loose tol_cost: near a minimum with a
    residual the relative decrease of a trial falls to 1e-8 and below, and its sign is then rounding's to decide.  The
    exact scenes stop on a loose tol_step for the same reason: a fourth trial would compare two costs of 1e-27, both
    rounding noise (test_posegraph_host.py asserts the margins of every trial of every case here).  Cached: the
    callers do not write into the scenes."""
    out = {"n1": (scene(1, 1), {}),
           "n2_exact": (scene(2, 1), STEP),
           "n3_exact": (scene(3, 1), STEP),
           "n30_exact": (scene(30, 1), STEP),
           "n43_exact": (scene(43, 1, "ring"), STEP),
           "n64_exact": (scene(64, 1, "ring"), STEP),
           "n3_noisy": (scene(3, 1, "all", True, 1), TWO),
           "n30_noisy": (scene(30, 1, "all", True, 5), TWO),
           "n30_noisy_tol": (scene(30, 1, "all", True, 5), dict(tol_cost=0.5)),
           "n30_noisy_cap": (scene(30, 1, "all", True, 5), dict(max_iters=1)),
           "n43_noisy": (scene(43, 1, "ring", True, 3), TWO),
           "n64_noisy": (scene(64, 1, "ring", True, 4), TWO),
           "n128_noisy": (scene(128, 1, "ring", True, 4), TWO),
           "reject": (scene(10, 1, "ring", True, 1, start=(100.0, 2.0)), dict(max_iters=8, tol_cost=0.0, tol_step=0.0)),
           "bad_edges": (with_bad_edges(scene(8, 1, "all", True, 0)), TWO),
           "disconnected": (disconnected(), TWO),
           "anchor3": (scene(8, 1, "all", True, 2), dict(TWO, anchor=3)),
           "zero_info": (zero_info(False), TWO),
           "zero_info_only_edge": (zero_info(True), dict(max_iters=4)),
           "cut_by_bad_edge": (cut_by_bad_edge(), TWO),
           "n1_bad_edges": (n1_bad_edges(), {})}
    full = scene(24, 1, "all", True, 0)
    for E in EDGE_COUNTS:
        out["edges_%d" % E] = (truncated(full, E), TWO)
    return out
