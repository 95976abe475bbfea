"""numpy restatement of the pose-graph refinement with a line process on the uncertain edges
(csrc/posegraph.hip mvr_posegraph_optimize_lp; DESIGN.md 4.22a, include/mvreg.h), and of the prune-and-repeat driver of
lib.multiview.optimize_pose_graph(line_process=True).  This file is the normative text of both; everything it does
not restate (conventions, residual, members, ignored edges, update, the trial) is tests/posegraph_oracle.py's.

    counted    an edge whose weight wc_k > 0 after the validity and membership rules of posegraph_oracle.edge_weights
    r_k        wc_k xi_k^T L_k xi_k
    mu         mu_scale * mean of L_k[0, 0] (the correspondence count) over the counted uncertain edges;
               mu_scale = preference_loop_closure * max_correspondence_distance^2
    l_k        s_k^2, s_k = mu / (mu + r_k), for a counted uncertain edge; 1 for a counted certain edge; reported as 0
               for an edge that does not count
    cost       c = sum_certain r_k + sum_uncertain l_k r_k + mu sum_uncertain (s_k - 1)^2, the three sums taken
               separately, each in edge order.  At the closed-form l this is the Geman-McClure cost
               sum_certain r_k + sum_uncertain mu r_k / (mu + r_k)
    start      l in closed form at the initial poses, c from it
    trial      H, g with the weights wc_k l_k, l held; the candidate's cost c' with the held l (and the held third sum);
               accept iff c' < c; on acceptance l is recomputed in closed form at the new poses from the r_k the
               candidate's cost pass formed, which gives c'' <= c'; the held cost becomes c'', lambda /= 10, and the
               tol_cost test is c - c'' <= tol_cost c.  On rejection lambda *= 10, l stays
    status 16  a counted uncertain edge exists but mu is not positive and finite: the scene runs with l = 1 on every
               counted edge (every edge certain)
With no uncertain edge counted the second and third sums are 0.0 and every weight is wc_k * 1.0: the loop is
posegraph_oracle.optimize's operation for operation.

Margins as posegraph_oracle: accept = |c - c'| / c, stop = the distance of each stop test's quantity from its
threshold (the tol_cost one on c - c'')."""
import functools

import numpy as np

import posegraph_oracle as PO

LINE_PROCESS_OFF = 16


def edge_costs(R, t, Rp, tp, ij, wc, L):
    """r_k [E], 0 where the edge does not count"""
    r = np.zeros(len(ij))
    for e in np.nonzero(wc > 0)[0]:
        i, j = ij[e]
        xi = PO.residual(R[i], t[i], R[j], t[j], Rp[e], tp[e])
        r[e] = wc[e] * (xi @ L[e] @ xi)
    return r


def _sum(x):
    c = 0.0
    for v in x:      # in edge order, one term at a time: what posegraph_oracle.cost does
        c += v
    return c


def closed_form(mu, r, unc):
    """-> l [E] (1 outside unc), the penalty mu sum_unc (s - 1)^2"""
    l = np.ones(len(r))
    s = mu / (mu + r[unc])
    l[unc] = s * s
    return l, mu * _sum((s - 1.0) ** 2)


def held_cost(r, l, pen, counted, unc):
    return _sum(r[counted & ~unc]) + _sum(l[unc] * r[unc]) + pen


def geman_mcclure(r, mu, counted, unc):
    return float(np.sum(r[counted & ~unc]) + np.sum(mu * r[unc] / (mu + r[unc])))


def optimize(R0, t0, Rp, tp, ij, info, w=None, uncertain=None, mu_scale=0.0025, anchor=0, max_iters=20, lambda0=1e-6,
             tol_cost=1e-9, tol_step=1e-10, solver="cholesky"):
    """One scene.  uncertain [E] (None: every edge).  -> the dict of posegraph_oracle.optimize plus line [E], mu,
    counted [E] bool, uncertain [E] bool (the counted uncertain edges the line process ran on), r [E] at the final
    poses."""
    R, t, Rp, tp, ij, w, info = PO._arrays(R0, t0, Rp, tp, ij, w, info)
    n, E = len(R), len(ij)
    flag = np.ones(E, bool) if uncertain is None else np.asarray(uncertain).reshape(-1) != 0
    trace = np.full(max_iters + 1, -1.0)
    out = {"R": R, "t": t, "member": np.zeros(n, np.int32), "cost": np.zeros(2), "iters": 0, "status": 0,
           "trace": trace, "accepted": [], "failed": [], "margins": [], "steps": [], "line": np.zeros(E), "mu": 0.0,
           "counted": np.zeros(E, bool), "uncertain": np.zeros(E, bool), "r": np.zeros(E)}
    if n == 0:
        out["status"] = 4 if E else 0
        return out
    if anchor >= n or not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        out["status"] = 4 | 1
        return out
    wc, member, ignored = PO.edge_weights(n, anchor, Rp, tp, ij, w, info)
    status = (4 if ignored else 0) | (1 if member.sum() < n else 0)
    L = np.nan_to_num(0.5 * (info + np.transpose(info, (0, 2, 1))))
    counted = wc > 0
    unc = counted & flag
    mu = 0.0
    if unc.any():
        mu = mu_scale * (_sum(L[unc, 0, 0]) / float(unc.sum()))
        if not (np.isfinite(mu) and mu > 0):
            status |= LINE_PROCESS_OFF
            unc = np.zeros(E, bool)
    r = edge_costs(R, t, Rp, tp, ij, wc, L)
    l, pen = closed_form(mu, r, unc)
    c = held_cost(r, l, pen, counted, unc)
    c_init = c
    trace[0] = c
    lam, k, converged, failed = lambda0, 0, c == 0.0, False
    while not converged and k < max_iters:
        H, g = PO.system(R, t, Rp, tp, ij, wc * l, L, member, anchor)
        M = H + lam * np.diag(np.diag(H))
        for f in range(n):
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
            Ex = PO.so3_exp(delta[6 * f + 3:6 * f + 6])
            Rc[f] = Ex @ R[f]
            tc[f] = Ex @ t[f] + delta[6 * f:6 * f + 3]
        rn = edge_costs(Rc, tc, Rp, tp, ij, wc, L)
        cn = held_cost(rn, l, pen, counted, unc)
        step = float(np.max(np.abs(delta)))
        accepted = cn < c
        m_accept = abs(c - cn) / c
        stops = [abs(step - tol_step) / max(tol_step, 1e-300)] if tol_step > 0 else []
        if accepted:
            l, pen = closed_form(mu, rn, unc)
            cn = held_cost(rn, l, pen, counted, unc)          # c'' <= c'
            if tol_cost > 0:
                stops.append(abs((c - cn) - tol_cost * c) / (tol_cost * c))
            if c - cn <= tol_cost * c:
                converged = True
            R, t, c, r = Rc, tc, cn, rn
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
    out.update(R=R, t=t, member=member, cost=np.array([c_init, c]), iters=k, status=status,
               line=np.where(counted, l, 0.0), mu=mu, counted=counted, uncertain=unc, r=r)
    return out


def run(sc, **kw):
    return optimize(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"],
                    sc.get("uncertain"), **kw)


def global_optimization(R0, t0, Rp, tp, ij, info, w=None, uncertain=None, mu_scale=0.0025,
                        edge_prune_threshold=0.25, prune_passes=2, **kw):
    """The driver of optimize_pose_graph(line_process=True): prune_passes times { optimise; give the uncertain edges
    with l < edge_prune_threshold weight 0; continue from the result }; prune_passes 0: one optimisation.
    -> the last pass's dict with line [E] (the l of the last optimisation in which the edge counted, 0 if in none),
    kept [E] bool (False for a pruned edge) and passes (the list of every pass's dict)."""
    E = len(np.asarray(ij).reshape(-1, 2))
    w = np.ones(E) if w is None else np.array(w, np.float64).reshape(-1)
    flag = np.ones(E, bool) if uncertain is None else np.asarray(uncertain).reshape(-1) != 0
    kept, line, passes = np.ones(E, bool), np.zeros(E), []
    R, t = R0, t0
    for p in range(max(int(prune_passes), 1)):
        out = optimize(R, t, Rp, tp, ij, info, w, flag, mu_scale, **kw)
        passes.append(out)
        line[out["counted"]] = out["line"][out["counted"]]
        if prune_passes > 0:
            drop = out["counted"] & flag & (out["line"] < edge_prune_threshold)
            w[drop] = 0.0
            kept[drop] = False
        R, t = out["R"], out["t"]
    res = dict(passes[-1])
    res.update(line=line, kept=kept, passes=passes)
    return res


# --------------------------------------------------------------------------------------------------- the test scenes
def with_outliers(sc, share, seed, keep_chain=True):
    """the scene with round(share * E) of its edges (of those with j != i + 1 when keep_chain) replaced by random
    transforms: a rotation by a uniform angle about a random axis, a translation uniform in [-2, 2]^3.
    -> (scene, bad [E] bool)"""
    rng = np.random.default_rng(seed)
    ij = np.asarray(sc["ij"])
    pool = np.nonzero(ij[:, 1] != ij[:, 0] + 1)[0] if keep_chain else np.arange(len(ij))
    n_bad = min(int(round(share * len(ij))), len(pool))
    bad = np.zeros(len(ij), bool)
    bad[rng.choice(pool, n_bad, replace=False)] = True
    out = dict(sc, R_pair=sc["R_pair"].copy(), t_pair=sc["t_pair"].copy())
    for e in np.nonzero(bad)[0]:
        out["R_pair"][e] = PO.random_rotation(rng)
        out["t_pair"][e] = rng.uniform(-2, 2, 3)
    return out, bad


def outlier_scene(n, seed, share, **kw):
    """posegraph_oracle.scene(n, seed, all pairs, noisy) with `share` outliers from seed + 100"""
    return with_outliers(PO.scene(n, seed, "all", True, 0, **kw), share, seed + 100)


def cost_evaluation_floor(sc, R, t, l, mu, anchor=0, seeds=(0, 1, 2)):
    """posegraph_oracle.cost_evaluation_floor for the held cost: how far the cost of one set of poses and one held l
    moves when the sum is evaluated another way (the edges in a shuffled order and in one sum, each term as
    xi . (w l L xi), the residual's products associated the other way round) -> the largest |difference|"""
    R, t, Rp, tp, ij, w, info = PO._arrays(R, t, sc["R_pair"], sc["t_pair"], sc["ij"], sc["w"], sc["info"])
    wc, _, _ = PO.edge_weights(len(R), anchor, Rp, tp, ij, w, info)
    L = np.nan_to_num(0.5 * (info + np.transpose(info, (0, 2, 1))))
    counted = wc > 0
    unc = counted & (l != 1.0)
    s = np.sqrt(l[unc])
    pen = mu * _sum((s - 1.0) ** 2)
    ref = held_cost(edge_costs(R, t, Rp, tp, ij, wc, L), l, pen, counted, unc)
    worst = 0.0
    for seed in seeds:
        c = 0.0
        for e in np.random.default_rng(seed).permutation(np.nonzero(counted)[0]):
            i, j = ij[e]
            D = (R[j].T @ R[i]) @ Rp[e].T
            xi = np.concatenate([R[j].T @ (t[i] - t[j]) - D @ tp[e], PO.so3_log(D)])
            c += xi @ ((wc[e] * l[e] * L[e]) @ xi)
        worst = max(worst, abs(c + pen - ref))
    return worst


def _extend(bad, sc):
    """the outlier mask of with_bad_edges(sc): its appended edges repeat edges 3, 5 (inverted) and 9; the ten between
    are ignored"""
    return np.concatenate([bad, [bad[3], bad[5]], np.zeros(PO.N_IGNORED, bool), [bad[9]]])


TRIALS = dict(max_iters=2, tol_cost=0.0, tol_step=0.0)
MU_SCALE = 0.0025          # preference_loop_closure 1, max_correspondence_distance 0.05
GLOBAL = dict(preference_loop_closure=1.0, max_correspondence_distance=0.05)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (scene (with `uncertain` where not every edge is), planted outliers [E] bool, keyword arguments of
    optimize, prune_passes): every scene test_gpu_posegraph_lp.py compares with this oracle through the driver.  Every
    pass runs a fixed number of trials (both tolerances 0), and the two-pass cases only two: the second pass starts
    near the first one's minimum, where a third trial's decrease falls to 3e-7 of the cost and a stop test would be
    rounding's to decide (test_posegraph_lp_host.py asserts every trial's margins and every edge's distance from the
    pruning threshold).  `long` and `reject` run one pass of more trials, the second on a ring with chords from a start
    100 degrees / 2 m off, for its four rejected trials.  Cached: the callers do not write into the scenes."""
    out = {}
    for name, (n, seed, share) in (("out6", (6, 1, 0.3)), ("out8", (8, 2, 0.4)), ("out30", (30, 1, 0.4))):
        out[name] = outlier_scene(n, seed, share) + (TRIALS, 2)
    full, bad = outlier_scene(24, 1, 0.3)
    for E in (255, 256, 257):
        out["edges_%d" % E] = (PO.truncated(full, E), bad[:E], TRIALS, 2)
    sc, bad = outlier_scene(8, 1, 0.3)
    out["chain_certain"] = (dict(sc, uncertain=(sc["ij"][:, 1] != sc["ij"][:, 0] + 1).astype(np.int32)), bad, TRIALS, 2)
    out["bad_edges"] = (PO.with_bad_edges(sc), _extend(bad, sc), TRIALS, 2)
    out["long"] = out["out8"][:2] + (dict(max_iters=6, tol_cost=0.0, tol_step=0.0), 1)
    far = PO.scene(10, 1, "ring", True, 1, start=(100.0, 2.0))
    out["reject"] = with_outliers(far, 0.3, 101) + (dict(max_iters=8, tol_cost=0.0, tol_step=0.0), 0)
    return out


def run_case(name, solver="cholesky"):
    sc, _, kw, passes = cases()[name]
    return global_optimization(sc["R0"], sc["t0"], sc["R_pair"], sc["t_pair"], sc["ij"], sc["info"], sc["w"],
                               sc.get("uncertain"), MU_SCALE, prune_passes=passes, solver=solver, **kw)


def disconnecting_scene(links=(5, 6)):
    """outlier_scene(8, 1, 0.3)'s fragments 0..6 with all their pairs, and fragment 7 reached only by the edges (i, 7),
    i in links, every one an outlier -> (scene, bad).  Two by default, because a fragment's only edge can always be met
    exactly and then has l = 1: a line process cannot tell that it is wrong (links=(6,): l = 0.94 after two trials).
    Two wrong edges that disagree are both far from met after the two trials of TRIALS and both go; run to convergence
    the fragment settles on one of them, which then stays"""
    sc, bad = outlier_scene(8, 1, 0.3)
    keep = [e for e, (i, j) in enumerate(sc["ij"]) if j != 7 or i in links]
    sc = dict(sc, R_pair=sc["R_pair"].copy(), t_pair=sc["t_pair"].copy())
    bad = bad.copy()
    rng = np.random.default_rng(7)
    for e, (i, j) in enumerate(sc["ij"]):
        if j == 7 and i in links:
            sc["R_pair"][e], sc["t_pair"][e] = PO.random_rotation(rng), rng.uniform(-2, 2, 3)
            bad[e] = True
    for k in ("R_pair", "t_pair", "ij", "info", "w"):
        sc[k] = sc[k][keep]
    return sc, bad[keep]


def zero_information_scene():
    """outlier_scene(6, 1, 0.3) with the chain edges certain and all-zero information on every other edge: mu = 0"""
    sc, _ = outlier_scene(6, 1, 0.3)
    unc = (sc["ij"][:, 1] != sc["ij"][:, 0] + 1).astype(np.int32)
    info = sc["info"].copy()
    info[unc != 0] = 0.0
    return dict(sc, info=info, uncertain=unc)
