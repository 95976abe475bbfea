"""Reference and case lists for the weighted Procrustes kernel (csrc/procrustes.hip) and its 3 x 3 SVD
(csrc/svd3.hpp) — TEST ORACLE ONLY, plain numpy.

kabsch_ld   lib/utils.py:164-237 (as restated in oracle/kabsch.py) with the sums taken two-pass in
            np.longdouble on the inputs rounded to `dtype`; the 3 x 3 SVD in fp64 (LAPACK).
feed        six points whose covariance is a given 3 x 3 matrix: any matrix reaches jacobi_svd3 through the
            public ABI.
*_cases     the inputs of tests/test_procrustes_host.py and tests/test_gpu_procrustes.py, from fixed seeds.

Matrices meant to be fed are kept on a dyadic grid (entries multiples of 2^-16, |entry| < 8) wherever the case
allows: every partial sum the kernel can form over feed(H) is then exact in fp64 IN ANY ORDER (the workgroup
reduction is a butterfly, not a left-to-right sum), the fp32 rounding of feed(H) is feed(H) itself, the
covariance the kernel solves is H bit for bit and the translation is exactly zero.  Rotation matrices cannot
lie on the grid (an orthogonal dyadic matrix is a signed permutation); tests bound their t instead.
"""
import functools

import numpy as np

LD = np.longdouble
GRID = 2.0 ** -16      # entries of a grid matrix
VGRID = 2.0 ** -8      # entries of the vectors whose outer products build the exactly rank-deficient ones
G_FLOOR = 0.05         # the conditioning every compared case must have; the generators ask for twice that
_G_GEN = 0.1


def _q(a, step):
    return np.round(np.asarray(a, np.float64) / step) * step


def on_grid(H):
    H = np.asarray(H, np.float64)
    return bool(np.all(H == _q(H, GRID)) and np.all(np.abs(H) < 8.0))


# ------------------------------------------------------------------------------------------------- reference
def kabsch_ld(x1, x2, w=None, normalize=True, eps=1e-7, dtype=np.float64):
    """x1, x2 [P, N, 3], w [P, N] or None (ones).  Returns a dict of fp64 arrays:
    R [P,3,3], t [P,3], mu1, mu2 [P,3], H [P,3,3] (the centred covariance sum w (x1-mu1)(x2-mu2)^T),
    s [P,3] (singular values, descending), d [P] (+-1), g [P] = (s1 + d s2) / s0 (0 for the zero matrix; the
    nearest rotation is unique iff g > 0), opt [P] = s0 + s1 + d s2 = max over rotations of tr(R H), and
    M [P] = sum w |x1| |x2|, the scale of the raw second moments."""
    dt = np.dtype(dtype)
    x1 = np.asarray(x1).astype(dt).astype(LD)
    x2 = np.asarray(x2).astype(dt).astype(LD)
    P, N, _ = x1.shape
    w = np.ones((P, N), LD) if w is None else np.asarray(w).astype(dt).astype(LD)
    e = LD(dt.type(eps))
    if normalize:                                                    # utils.py:187-189
        w = w / (w.sum(axis=1, keepdims=True) + e)
    den = w.sum(axis=1)[:, None] + e                                 # utils.py:203-204
    mu1 = (w[:, :, None] * x1).sum(axis=1) / den
    mu2 = (w[:, :, None] * x2).sum(axis=1) / den
    x1c = x1 - mu1[:, None, :]
    x2c = x2 - mu2[:, None, :]
    H = np.einsum("pn,pni,pnj->pij", w, x1c, x2c)
    M = (w * np.sqrt((x1 * x1).sum(-1)) * np.sqrt((x2 * x2).sum(-1))).sum(axis=1)
    out = {k: np.empty(s) for k, s in (("R", (P, 3, 3)), ("t", (P, 3)), ("s", (P, 3)), ("d", P), ("g", P),
                                       ("opt", P))}
    out.update(mu1=mu1.astype(np.float64), mu2=mu2.astype(np.float64), H=H.astype(np.float64),
               M=M.astype(np.float64))
    for p in range(P):
        u, s, vh = np.linalg.svd(out["H"][p])                        # utils.py:214 (torch.svd: cov = U S V^T)
        v = vh.T
        d = -1.0 if np.linalg.det(v @ u.T) < 0 else 1.0              # utils.py:225-227
        R = v @ np.diag([1.0, 1.0, d]) @ u.T                         # utils.py:229
        out["R"][p], out["s"][p], out["d"][p] = R, s, d
        out["t"][p] = (mu2[p] - R.astype(LD) @ mu1[p]).astype(np.float64)   # utils.py:232
        out["g"][p] = (s[1] + d * s[2]) / s[0] if s[0] > 0 else 0.0
        out["opt"][p] = s[0] + s[1] + d * s[2]
    return out


def feed(H):
    """H [M,3,3] -> x1, x2 [M,6,3] with sum_n x1_n x2_n^T = H and both sums zero: x1 = (+e0, +e1, +e2, -e0, -e1,
    -e2), x2 = (+H[0]/2, +H[1]/2, +H[2]/2, -H[0]/2, -H[1]/2, -H[2]/2).  Call with w = NULL, normalize = 0,
    eps = 0."""
    H = np.asarray(H, np.float64).reshape(-1, 3, 3)
    e = np.concatenate([np.eye(3), -np.eye(3)])
    x1 = np.broadcast_to(e, (H.shape[0], 6, 3)).copy()
    x2 = np.concatenate([H / 2, -H / 2], axis=1)
    return x1, x2


def solve_fed(H, dtype=np.float64):
    """kabsch_ld on feed(H)"""
    x1, x2 = feed(H)
    return kabsch_ld(x1, x2, None, False, 0.0, dtype)


def rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def _gap(H):
    return float(solve_fed(H)["g"][0])


def _draw(rng, make, ok=lambda H: True):
    """the first matrix of the stream make(rng) that is well conditioned (and ok)"""
    for _ in range(1000):
        H = make(rng)
        if _gap(H) >= _G_GEN and ok(H):
            return H
    raise RuntimeError("no well-conditioned draw")


# ---------------------------------------------------------------------------------- A: unique solves via feed
@functools.lru_cache(maxsize=None)
def svd_unique_cases():
    """(H [93,3,3], kinds): every matrix has g >= G_FLOOR, so R is unique.  kinds[i] is one of 'gauss+',
    'gauss-' (det < 0: the d = -1 branch), 'diag', 'rot', 'rank2', 'zerocol', 'zerorow'."""
    rng = np.random.default_rng(20240)
    Hs, kinds = [], []
    gauss = lambda r: _q(np.clip(r.standard_normal((3, 3)), -7.5, 7.5), GRID)   # noqa: E731
    for sign, kind in ((1, "gauss+"), (-1, "gauss-")):
        for _ in range(32):
            Hs.append(_draw(rng, gauss, lambda H: np.linalg.det(H) * sign > 0))
            kinds.append(kind)
    for dg in ((1, 2, 3), (3, 2, 1), (2, 3, 1), (1, 2, -3), (-3, 1, 2)):
        Hs.append(np.diag(np.asarray(dg, np.float64)))
        kinds.append("diag")
    for _ in range(8):
        Hs.append(rotation(rng))
        kinds.append("rot")

    def rank2(r):
        U, V = rotation(r), rotation(r)
        s0, s1 = r.uniform(1.0, 3.0), r.uniform(0.5, 1.0)
        return (np.outer(_q(s0 * U[:, 0], VGRID), _q(V[:, 0], VGRID))
                + np.outer(_q(s1 * U[:, 1], VGRID), _q(V[:, 1], VGRID)))
    for _ in range(8):
        Hs.append(_draw(rng, rank2))
        kinds.append("rank2")
    for kind, axis in (("zerocol", 1), ("zerorow", 0)):
        for k in range(4):
            def zeroed(r, k=k, axis=axis):
                H = gauss(r)
                H[tuple([slice(None)] * axis + [k % 3])] = 0.0
                return H
            Hs.append(_draw(rng, zeroed))
            kinds.append(kind)
    H = np.stack(Hs)
    H.setflags(write=False)
    return H, tuple(kinds)


# ------------------------------------------------------------------------------- B: non-unique solves via feed
@functools.lru_cache(maxsize=None)
def svd_nonunique_cases():
    """(H [15,3,3], kinds): the maximiser of tr(R H) over rotations is not unique; only its value is."""
    rng = np.random.default_rng(20241)
    e = np.eye(3)
    Hs = [2.0 * np.outer(e[0], e[0]), np.outer(e[1], e[2]), 0.5 * np.outer(e[2], e[0])]
    for _ in range(5):
        Hs.append(np.outer(_q(rng.uniform(0.5, 3.0) * rotation(rng)[:, 0], VGRID), _q(rotation(rng)[:, 0], VGRID)))
    kinds = ["rank1"] * 8
    Hs += [np.zeros((3, 3)), -np.eye(3), np.diag([2.0, 1.0, -1.0])]
    kinds += ["zero", "-I", "diag(2,1,-1)"]
    for _ in range(4):
        Q, Pm = rotation(rng), rotation(rng)
        Hs.append(-(Q @ np.diag([2.0, 1.0, 1.0]) @ Pm))              # det = -2
        kinds.append("Q diag(2,1,1) P, det < 0")
    H = np.stack(Hs)
    H.setflags(write=False)
    return H, tuple(kinds)


# ------------------------------------------------------------------------------------ C: reduction shapes
REDUCTION_N = (1, 2, 3, 4, 255, 256, 257, 1023)


def _noisy_pairs(rng, P, N, offset=0.0, noise=0.01):
    x1 = np.empty((P, N, 3))
    x2 = np.empty((P, N, 3))
    for p in range(P):
        u = rng.standard_normal(3)
        x1[p] = offset * u / np.linalg.norm(u) + rng.standard_normal((N, 3))
        x2[p] = x1[p] @ rotation(rng).T + rng.standard_normal(3) + noise * rng.standard_normal((N, 3))
    return x1, x2


@functools.lru_cache(maxsize=None)
def reduction_case(N):
    """(x1, x2 [3,N,3], w [3,N]): weights in (0.1, 1), N // 4 of each row exactly 0; for N >= 3 every pair is
    drawn until g >= 0.1 in both precisions (three weighted points can be nearly collinear)."""
    rng = np.random.default_rng(7000 + N)
    for _ in range(1000):
        x1, x2 = _noisy_pairs(rng, 3, N)
        w = rng.uniform(0.1, 1.0, (3, N))
        for p in range(3):
            w[p, rng.permutation(N)[:N // 4]] = 0.0
        if N < 3 or min(kabsch_ld(x1, x2, w, True, 1e-7, dt)["g"].min() for dt in (np.float64, np.float32)) >= _G_GEN:
            for a in (x1, x2, w):
                a.setflags(write=False)
            return x1, x2, w
    raise RuntimeError("no well-conditioned draw")


# --------------------------------------------------------------------------------------- D: far from origin
FAR_C = {np.dtype(np.float64): (1e2, 1e3, 1e4), np.dtype(np.float32): (1e2, 1e3)}


@functools.lru_cache(maxsize=None)
def far_case(c):
    """(x1, x2 [4,257,3], w [4,257]): spread 1, noise 0.01, the cloud c away from the origin"""
    rng = np.random.default_rng(9000 + int(round(np.log10(c))))
    x1, x2 = _noisy_pairs(rng, 4, 257, offset=c)
    w = rng.uniform(0.1, 1.0, (4, 257))
    for a in (x1, x2, w):
        a.setflags(write=False)
    return x1, x2, w


# ------------------------------------------------------------------------------------------ E, F: status, scale
@functools.lru_cache(maxsize=None)
def plain_case(N=300):
    """(x1, x2 [3,N,3], w [3,N]) near the origin, for the status and the scaling tests"""
    rng = np.random.default_rng(11000 + N)
    x1, x2 = _noisy_pairs(rng, 3, N)
    w = rng.uniform(0.1, 1.0, (3, N))
    for a in (x1, x2, w):
        a.setflags(write=False)
    return x1, x2, w


# ------------------------------------------------------------------------------------------- property checks
def rotation_defects(R):
    """(max |R^T R - I|, |det R - 1|) of one 3 x 3 matrix, in fp64"""
    R = np.asarray(R, np.float64)
    return float(np.abs(R.T @ R - np.eye(3)).max()), float(abs(np.linalg.det(R) - 1.0))


def trace_gain(R, H):
    """tr(R H) = sum_n x2_n . R x1_n over the centred points: what Kabsch maximises"""
    return float(np.trace(np.asarray(R, np.float64) @ np.asarray(H, np.float64)))
