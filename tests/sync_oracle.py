"""numpy restatement of the multiview pose synchronisation (csrc/sync.hip mvr_sync_poses) and a scene generator.

The reference never released this stage, so there is no reference code to compare with: parity is pinned to the
closed form stated below and to ground truth.  The restatement uses
np.linalg.eigh / svd / solve; the kernel reaches the same subspace by inverse subspace iteration.

Conventions.  Edge k = (i, j, R_k, t_k, w_k) with x_j ~ R_k x_i + t_k; poses (R_i, t_i) with X = R_i x_i + t_i in
a common frame, so R_k = R_j^T R_i and R_j t_k = t_i - t_j; gauge R_a = I, t_a = 0 for the anchor a.
  1. members: fragments reachable from a over edges with w > 0; other edges get weight 0, other fragments come
     out as R = I, t = 0, member = 0.
  2. rotations: L (3N x 3N): block (j,i) -= w R_k, (i,j) -= w R_k^T, (i,i) and (j,j) += w I, non-member diagonal
     blocks += max(1, 2 sum w) I.  U = eigenvectors of the 3 smallest eigenvalues; if the members' sum of
     sign(det U_i) < 0 negate U's third column; V_i = proj(U_i)^T with proj(M) = A diag(1, 1, det(A B^T)) B^T of
     the SVD M = A S B^T; R_i = V_a^T V_i.
  3. translations: weighted graph Laplacian A, b_i += w R_j t_k, b_j -= w R_j t_k; the anchor and the
     non-members deleted, A t = b solved, t_a = 0.
  4. residuals: e_k = |R_k - R_j^T R_i|_F, d_k = |t_i - t_j - R_j t_k|_2.
  5. IRLS: w_k <- w0_k / (1 + (e_k / c_rot)^2) / (1 + (d_k / c_trans)^2), steps 1-4 again (members from w0 only).
status bits: 1 some fragment is not a member; 2 never (the kernel's iteration cap); 4 an edge was ignored (index
out of range or i == j, a non-finite value, a negative weight) or anchor >= n_frags (whole scene identity).
Ignored edges come out with weight 0 and residuals 0.
"""
import numpy as np


def proj_so3(M):
    A, _, Bt = np.linalg.svd(M)
    return A @ np.diag([1.0, 1.0, np.linalg.det(A @ Bt)]) @ Bt


def _members(n, ij, w, anchor):
    m = np.zeros(n, bool)
    m[anchor] = True
    changed = True
    while changed:
        changed = False
        for (i, j), wk in zip(ij, w):
            if wk > 0 and m[i] != m[j]:
                m[i] = m[j] = True
                changed = True
    return m


def rotation_laplacian(R_pair, ij, w, member):
    n = len(member)
    L = np.zeros((3 * n, 3 * n))
    for (i, j), Rk, wk in zip(ij, R_pair, w):
        L[3 * j:3 * j + 3, 3 * i:3 * i + 3] -= wk * Rk
        L[3 * i:3 * i + 3, 3 * j:3 * j + 3] -= wk * Rk.T
        L[3 * i:3 * i + 3, 3 * i:3 * i + 3] += wk * np.eye(3)
        L[3 * j:3 * j + 3, 3 * j:3 * j + 3] += wk * np.eye(3)
    pad = max(1.0, 2.0 * float(np.sum(w)))
    for f in np.nonzero(~member)[0]:
        L[3 * f:3 * f + 3, 3 * f:3 * f + 3] += pad * np.eye(3)
    return L


def _solve_once(R_pair, t_pair, ij, w, member, anchor):
    n = len(member)
    L = rotation_laplacian(R_pair, ij, w, member)
    lam, vec = np.linalg.eigh(L)
    U = vec[:, :3].copy()
    s = sum(np.sign(np.linalg.det(U[3 * f:3 * f + 3])) for f in np.nonzero(member)[0])
    if s < 0:
        U[:, 2] = -U[:, 2]
    V = [proj_so3(U[3 * f:3 * f + 3]).T for f in range(n)]
    R = np.tile(np.eye(3), (n, 1, 1))
    for f in np.nonzero(member)[0]:
        R[f] = V[anchor].T @ V[f]
    R[anchor] = np.eye(3)
    A = np.zeros((n, n))
    b = np.zeros((n, 3))
    for (i, j), tk, wk in zip(ij, t_pair, w):
        c = wk * (R[j] @ tk)
        A[i, i] += wk
        A[j, j] += wk
        A[i, j] -= wk
        A[j, i] -= wk
        b[i] += c
        b[j] -= c
    keep = [f for f in range(n) if member[f] and f != anchor]
    t = np.zeros((n, 3))
    if keep:
        t[keep] = np.linalg.solve(A[np.ix_(keep, keep)], b[keep])
    return R, t, lam


def residuals(R_pair, t_pair, ij, R, t):
    e = np.array([np.linalg.norm(Rk - R[j].T @ R[i]) for (i, j), Rk in zip(ij, R_pair)]).reshape(-1)
    d = np.array([np.linalg.norm(t[i] - t[j] - R[j] @ tk) for (i, j), tk in zip(ij, t_pair)]).reshape(-1)
    return e, d


def sync_oracle(R_pair, t_pair, ij, n_frags, w=None, anchor=0, irls_iters=0, c_rot=0.1, c_trans=0.1,
                return_spectrum=False):
    """One scene.  R_pair [E,3,3], t_pair [E,3], ij [E,2], w [E] or None -> dict of R [N,3,3], t [N,3], member [N]
    int32, weights / res_rot / res_trans [E], status int (and, asked for, the spectrum of every pass's L)."""
    R_pair = np.asarray(R_pair, np.float64).reshape(-1, 3, 3)
    t_pair = np.asarray(t_pair, np.float64).reshape(-1, 3)
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    E, n = len(ij), int(n_frags)
    w0 = np.ones(E) if w is None else np.asarray(w, np.float64).reshape(-1).copy()
    out = {"R": np.tile(np.eye(3), (n, 1, 1)), "t": np.zeros((n, 3)), "member": np.zeros(n, np.int32),
           "weights": np.zeros(E), "res_rot": np.zeros(E), "res_trans": np.zeros(E), "status": 0}
    if n == 0:
        return out
    if anchor >= n:
        out["status"] = 4 | 1
        return out
    ok = ((ij[:, 0] >= 0) & (ij[:, 0] < n) & (ij[:, 1] >= 0) & (ij[:, 1] < n) & (ij[:, 0] != ij[:, 1]) &
          np.isfinite(R_pair).all((1, 2)) & np.isfinite(t_pair).all(1) & np.isfinite(w0))
    ok &= np.where(np.isfinite(w0), w0, 0.0) >= 0
    status = 0 if ok.all() else 4
    idx = np.nonzero(ok)[0]
    Rp, tp, e_ij, w0v = R_pair[idx], t_pair[idx], ij[idx], w0[idx]
    member = _members(n, e_ij, w0v, anchor)
    if not member.all():
        status |= 1
    w0v = np.where(member[e_ij[:, 0]] & member[e_ij[:, 1]], w0v, 0.0) if len(idx) else w0v
    wv = w0v.copy()
    spectra = []
    for it in range(irls_iters + 1):
        R, t, lam = _solve_once(Rp, tp, e_ij, wv, member, anchor)
        spectra.append(lam)
        e, d = residuals(Rp, tp, e_ij, R, t) if len(idx) else (np.zeros(0), np.zeros(0))
        if it < irls_iters:
            wv = w0v / (1.0 + (e / c_rot) ** 2) / (1.0 + (d / c_trans) ** 2)
    out.update(R=R, t=t, member=member.astype(np.int32), status=status)
    out["weights"][idx], out["res_rot"][idx], out["res_trans"][idx] = wv, e, d
    if return_spectrum:
        out["spectra"] = spectra
    return out


# ---------------------------------------------------------------------------------------------- scene generator
def rodrigues(v):
    th = np.linalg.norm(v)
    if th < 1e-300:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def complete_edges(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def ring_edges(n):
    return [(i, (i + 1) % n) for i in range(n)]


def chain_edges_reversed(n):
    """n - 1 edges of a chain, sources and targets reversed (i > j)"""
    return [(i + 1, i) for i in range(n - 1)]


def make_scene(n, edges, seed=0, sigma_rot=0.0, sigma_t=0.0, outlier_share=0.0, anchor=0, random_weights=False):
    """Random ground-truth poses gauged to `anchor` and the edges they imply, with optional noise (rotation: a
    right-multiplied axis-angle vector of standard deviation sigma_rot; translation: sigma_t) and a share of edges
    replaced by random transforms.  Returns dict R_gt, t_gt, R_pair, t_pair, ij, w, outlier (bool [E])."""
    rng = np.random.default_rng(seed)
    Rg = np.stack([random_rotation(rng) for _ in range(n)])
    tg = rng.uniform(-2.0, 2.0, (n, 3))
    Ra, ta = Rg[anchor].copy(), tg[anchor].copy()
    tg = (tg - ta) @ Ra              # rows: Ra^T (t_i - t_a)
    Rg = np.stack([Ra.T @ r for r in Rg])
    ij = np.asarray(edges, np.int64).reshape(-1, 2)
    E = len(ij)
    outlier = np.zeros(E, bool)
    if outlier_share > 0:
        outlier[rng.choice(E, int(round(outlier_share * E)), replace=False)] = True
    Rp, tp = np.zeros((E, 3, 3)), np.zeros((E, 3))
    for k, (i, j) in enumerate(ij):
        if outlier[k]:
            Rp[k], tp[k] = random_rotation(rng), rng.uniform(-2.0, 2.0, 3)
            continue
        Rp[k] = Rg[j].T @ Rg[i] @ rodrigues(sigma_rot * rng.standard_normal(3))
        tp[k] = Rg[j].T @ (tg[i] - tg[j]) + sigma_t * rng.standard_normal(3)
    w = rng.uniform(0.2, 1.0, E) if random_weights else np.ones(E)
    return {"n": n, "anchor": anchor, "R_gt": Rg, "t_gt": tg, "R_pair": Rp, "t_pair": tp, "ij": ij, "w": w,
            "outlier": outlier}


def pose_error(out, scene, member=None):
    """worst rotation (Frobenius) and translation (L2) error over the member fragments"""
    m = np.ones(scene["n"], bool) if member is None else np.asarray(member, bool)
    er = np.linalg.norm(out["R"][m] - scene["R_gt"][m], axis=(1, 2)).max()
    et = np.linalg.norm(out["t"][m] - scene["t_gt"][m], axis=1).max()
    return float(er), float(et)


def spectral_gap(spectrum):
    """(lambda_4 - lambda_3) / lambda_max of one pass's L"""
    return float((spectrum[3] - spectrum[2]) / spectrum[-1])


# ------------------------------------------------------------------------- the scenes the CPU and GPU tests share
def _with_bad_edges(scene):
    """two edges appended that must be ignored: one with i == j, one with a NaN rotation entry"""
    s = dict(scene)
    bad_R = np.stack([np.eye(3), np.eye(3)])
    bad_R[1, 0, 0] = np.nan
    s["R_pair"] = np.concatenate([scene["R_pair"], bad_R])
    s["t_pair"] = np.concatenate([scene["t_pair"], np.zeros((2, 3))])
    s["ij"] = np.concatenate([scene["ij"], np.array([[2, 2], [0, 3]])])
    s["w"] = np.concatenate([scene["w"], np.ones(2)])
    s["outlier"] = np.concatenate([scene["outlier"], np.zeros(2, bool)])
    return s


def _cut_by_bad_edge(scene):
    """a chain (0,1), (1,2) whose second edge gets a NaN in its rotation, and a self-loop (2,2) appended: the ignored
    edge is the only way to fragment 2, so the edge test decides the component"""
    s = dict(scene)
    s["R_pair"] = np.concatenate([scene["R_pair"], np.eye(3)[None]])
    s["R_pair"][1, 0, 2] = np.nan
    s["t_pair"] = np.concatenate([scene["t_pair"], np.zeros((1, 3))])
    s["ij"] = np.concatenate([scene["ij"], np.array([[2, 2]])])
    s["w"] = np.concatenate([scene["w"], np.ones(1)])
    s["outlier"] = np.concatenate([scene["outlier"], np.zeros(1, bool)])
    return s


CASES = {
    # name: (scene constructor, irls passes)
    "n2": (lambda: make_scene(2, [(0, 1)], 1), 0),
    "n3": (lambda: make_scene(3, complete_edges(3), 2), 0),
    "complete30": (lambda: make_scene(30, complete_edges(30), 3), 0),
    "ring12": (lambda: make_scene(12, ring_edges(12), 4), 0),
    "chain12_reversed": (lambda: make_scene(12, chain_edges_reversed(12), 5), 0),
    "complete30_noisy": (lambda: make_scene(30, complete_edges(30), 6, 0.02, 0.02, random_weights=True), 0),
    "ring12_noisy": (lambda: make_scene(12, ring_edges(12), 7, 0.02, 0.02, random_weights=True), 0),
    "anchor7": (lambda: make_scene(30, complete_edges(30), 8, 0.02, 0.02, anchor=7, random_weights=True), 0),
    "outliers30": (lambda: make_scene(30, complete_edges(30), 11, 0.01, 0.01, 0.3), 5),
    # fragments {0,1,2} and {3,4,5} form two components, 6 and 7 are isolated
    "two_components": (lambda: make_scene(8, [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3)], 10), 0),
    "bad_edges": (lambda: _with_bad_edges(make_scene(6, complete_edges(6), 12, 0.02, 0.02)), 0),
    "cut_by_bad_edge": (lambda: _cut_by_bad_edge(make_scene(3, [(0, 1), (1, 2)], 15, 0.02, 0.02)), 2),
    "complete64": (lambda: make_scene(64, complete_edges(64), 9, 0.02, 0.02, random_weights=True), 0),
    # either side of the kernel's switch from the LDS-resident to the workspace-resident matrix (max_frags 42 | 43)
    "complete42": (lambda: make_scene(42, complete_edges(42), 13, 0.02, 0.02, random_weights=True), 0),
    "complete43": (lambda: make_scene(43, complete_edges(43), 14, 0.02, 0.02, random_weights=True), 0),
}
# one fragment with two edges that cannot count, (0,0) and (0,1): status 4, nothing solved.  Not in CASES: a single
# fragment has no spectrum
N1_BAD_EDGES = {"n": 1, "anchor": 0, "R_pair": np.tile(np.eye(3), (2, 1, 1)), "t_pair": np.zeros((2, 3)),
                "ij": np.array([[0, 0], [0, 1]], np.int64), "w": np.ones(2)}
NOISE_FREE = ("n2", "n3", "complete30", "ring12", "chain12_reversed")
OUTLIER_BOUND = 0.05   # the outlier scenes: 5 IRLS passes land within it, 0 passes do not

_cache = {}


def case(name):
    """(scene, irls passes, the oracle's result with every pass's spectrum), computed once per process"""
    if name not in _cache:
        make, irls = CASES[name]
        sc = make()
        out = sync_oracle(sc["R_pair"], sc["t_pair"], sc["ij"], sc["n"], sc["w"], sc["anchor"], irls,
                          return_spectrum=True)
        _cache[name] = (sc, irls, out)
    return _cache[name]
