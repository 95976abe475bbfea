"""Byte comparison of two builds of the library on what csrc/ransac.hpp's users compute: mvr_ransac, mvr_ransac_checked
(csrc/ransac.hip) and mvr_fgr (csrc/fgr.hip).  The oracles pin the selection bit for bit but the fits to 1e-9 only; a
change that must not move a bit is shown against the build before it.
For each library one fresh child process (MVR_LIB selects the library) runs the cases and writes every output to an
.npz; this process, which never opens the GPU, then compares the two files key by key with tobytes():
  * mvr_ransac with hyp_out at ransac_n 3, 4 and 8 over tests/test_gpu_ransac_checked.py's anchor inputs
    (parity_inputs(300) at 256 iterations, parity_inputs(37) at 100, plus a pair of 2 rows);
  * mvr_ransac_checked on the same, checkers off (cap = iterations) and edge 0.9 + distance 0.05 at cap 64;
  * mvr_fgr at its defaults on tests/fgr_oracle.py's batch, tuple filter on and off, with the trace.
usage: python tools/ransac_ab.py LIB_A LIB_B [--keep DIR]     exit status 0: every key identical"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d_multiview_reg_amd"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

SENT = -77
SHAPES = [(300, 256), (37, 100)]


def child(out_path):
    import torch
    import fgr_oracle as F
    import ransac_checked_oracle as C
    from lib import _native as N
    d = torch.device("cuda")
    L = N.lib()
    out = {}
    f64 = lambda *s: torch.full(s, float(SENT), dtype=torch.float64, device=d)   # noqa: E731
    i32 = lambda *s: torch.full(s, SENT, dtype=torch.int32, device=d)            # noqa: E731

    def keep(tag, o):
        torch.cuda.synchronize()
        for k, v in o.items():
            out[tag + " " + k] = v.cpu().numpy()

    for n, iters in SHAPES:
        (x1, x2), counts = C.parity_inputs(n)
        counts = counts + [2]
        x1, x2 = np.concatenate([x1, x1[:1]]), np.concatenate([x2, x2[:1]])
        P = len(counts)
        X1, X2 = torch.from_numpy(x1).to(d), torch.from_numpy(x2).to(d)
        cnt = torch.tensor(counts, dtype=torch.int32, device=d)
        for rn in (3, 4, 8):
            # rows of a pair below ransac_n keep the sentinel in hyp: written by neither build
            o = {"T": f64(P, 4, 4), "fitness": f64(P), "rmse": f64(P), "best_iter": i32(P), "hyp": f64(P, iters, 12)}
            ws = torch.empty(L.mvr_ransac_workspace_bytes(P, iters), dtype=torch.uint8, device=d)
            N.check(L.mvr_ransac(N.ptr(X1), N.ptr(X2), n * 3, N.ptr(cnt), P, rn, iters, C.MAX_DIST, C.SEED,
                                 N.ptr(o["T"]), N.ptr(o["fitness"]), N.ptr(o["rmse"]), N.ptr(o["best_iter"]),
                                 N.ptr(o["hyp"]), N.ptr(ws), ws.numel(), N.stream()), "mvr_ransac")
            keep("ransac n%d i%d k%d" % (n, iters, rn), o)
            for mode, edge, dist, cap in (("off", 0.0, 0.0, iters), ("edge+dist", 0.9, C.MAX_DIST, 64)):
                nw = (iters + 63) // 64
                o = {"T": f64(P, 4, 4), "fitness": f64(P), "rmse": f64(P), "best_iter": i32(P), "n_pass": i32(P),
                     "n_valid": i32(P), "words": torch.full((P, nw), SENT, dtype=torch.int64, device=d),
                     "valid": i32(P, cap), "hyp": f64(P, cap, 12)}
                ws = torch.empty(L.mvr_ransac_checked_workspace_bytes(P, iters, cap), dtype=torch.uint8, device=d)
                N.check(L.mvr_ransac_checked(N.ptr(X1), N.ptr(X2), n * 3, N.ptr(cnt), P, rn, iters, C.MAX_DIST,
                                             C.SEED, cap, edge, dist, None, None, -1.0, N.ptr(o["T"]),
                                             N.ptr(o["fitness"]), N.ptr(o["rmse"]), N.ptr(o["best_iter"]),
                                             N.ptr(o["n_pass"]), N.ptr(o["n_valid"]), N.ptr(o["words"]),
                                             N.ptr(o["valid"]), N.ptr(o["hyp"]), N.ptr(ws), ws.numel(), N.stream()),
                        "mvr_ransac_checked")
                keep("checked %s n%d i%d k%d" % (mode, n, iters, rn), o)

    x1, x2, counts = F.batch()
    P, n = x1.shape[0], x1.shape[1]
    X1, X2 = torch.from_numpy(x1.copy()).to(d), torch.from_numpy(x2.copy()).to(d)   # the batch is read-only
    cnt = torch.from_numpy(counts).to(d)
    q = F.DEFAULTS
    for tuple_test in (True, False):
        o = {"T": f64(P, 4, 4), "fitness": f64(P), "rmse": f64(P), "n_used": i32(P), "n_tuples": i32(P),
             "status": i32(P), "trace": f64(P, q["iters"], 2)}
        ws = torch.empty(L.mvr_fgr_workspace_bytes(P, n, q["max_tuples"]), dtype=torch.uint8, device=d)
        N.check(L.mvr_fgr(N.ptr(X1), N.ptr(X2), 3 * n, N.ptr(cnt), P, q["max_dist"], q["iters"], q["division_factor"],
                          q["tuple_factor"] if tuple_test else 0, q["max_tuples"], q["tuple_scale"], F.SEED,
                          N.ptr(o["T"]), N.ptr(o["fitness"]), N.ptr(o["rmse"]), N.ptr(o["n_used"]),
                          N.ptr(o["n_tuples"]), N.ptr(o["status"]), N.ptr(o["trace"]), N.ptr(ws), ws.numel(),
                          N.stream()), "mvr_fgr")
        keep("fgr tuple_test=%s" % tuple_test, o)
    np.savez(out_path, **out)
    print("%s (%s): %d arrays" % (N.LIB_PATH, N.source_hash(), len(out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--keep", help="directory for the two .npz files (default: a temporary one)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if len(a.libs) != 2:
        ap.error("two libraries")
    with tempfile.TemporaryDirectory() as tmp:
        where = a.keep or tmp
        os.makedirs(where, exist_ok=True)
        files = []
        for tag, lib in zip("ab", a.libs):
            files.append(os.path.join(where, "ransac_ab_%s.npz" % tag))
            env = dict(os.environ, MVR_LIB=os.path.abspath(lib))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", files[-1]], env=env, check=True,
                           timeout=300)
        A, B = (dict(np.load(f)) for f in files)
    bad = sorted(set(A) ^ set(B))
    for k in sorted(set(A) & set(B)):
        if A[k].dtype != B[k].dtype or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes():
            bad.append(k)
    written = sum(int((v != SENT).sum()) for v in A.values())
    print("%d keys, %d bytes, %d values written: %s" % (len(A), sum(v.nbytes for v in A.values()), written,
                                                        "all identical" if not bad else "DIFFERENT: " + ", ".join(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
