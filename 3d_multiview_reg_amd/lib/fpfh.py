"""Weights-free global registration: FPFH descriptors (csrc/fpfh.hip mvr_compute_fpfh, FragmentOverlap.compute_fpfh),
nearest neighbours in feature space (csrc/feat_match.hip mvr_feat_match) and the batched RANSAC (mvr_ransac,
lib.utils.run_ransac_batch) or Fast Global Registration (mvr_fgr, lib.utils.run_fgr_batch; register_fgr, DESIGN.md
4.28); DESIGN.md 4.24, the semantics are in include/mvreg.h.

What Open3D users write as compute_fpfh_feature + registration_ransac_based_on_feature_matching, for every pair of a
scene at once and without a pretrained network: a coarse estimate that feeds lib.icp.icp_refine / gicp_refine and
lib.multiview.synchronize unchanged.  Restated from the maths; Open3D parity is unpinned.

Convention: T maps source coordinates into the target's frame, x_target ~ T x_source (lib/icp.py)."""
import numpy as np
import torch

from lib import _native as N
from lib.utils import RANSAC_DIST, RANSAC_ITERS, RANSAC_N, run_fgr_batch, run_ransac_batch, run_ransac_checked_batch

MAX_CHANNELS = 64


def _check_inputs(name, feats, off, pairs):
    if not torch.is_tensor(feats) or feats.dim() != 2 or feats.dtype != torch.float32:
        raise ValueError("%s: feats must be a fp32 [M,C] tensor" % name)
    if not 1 <= feats.shape[1] <= MAX_CHANNELS:
        raise ValueError("%s: %d channels; mvr_feat_match takes 1..%d" % (name, feats.shape[1], MAX_CHANNELS))
    off = np.asarray(off, dtype=np.int64).reshape(-1)
    if len(off) < 2 or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != feats.shape[0]:
        raise ValueError("%s: off must be the [B+1] prefix sums of the fragments' sizes, ending at M" % name)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= len(off) - 1):
        raise ValueError("%s: pairs holds a fragment index outside [0, %d)" % (name, len(off) - 1))
    return off, pairs


def feat_match(feats, off, pairs):
    """mvr_feat_match: for every row of a pair's query fragment the nearest row of its target fragment in feature
    space.  feats fp32 [M,C] on the device (C <= 64), off [B+1] host, pairs [P,2] (query fragment, target fragment).
    -> (idx int32 [Q] device: rows within the target fragment, -1 for an empty target; dist2 fp32 [Q] device;
    qoff int64 [P+1] numpy: pair p's queries are idx[qoff[p]:qoff[p+1]])"""
    off, pairs = _check_inputs("feat_match", feats, off, pairs)
    N.require_hip(feats)
    feats = feats.contiguous()
    dev = feats.device
    P = len(pairs)
    nq = np.diff(off)[pairs[:, 0]] if P else np.zeros(0, np.int64)
    qoff = np.concatenate([[0], np.cumsum(nq)]).astype(np.int64)
    Q = int(qoff[-1])
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    dist2 = torch.empty(Q, dtype=torch.float32, device=dev)
    if Q:
        g_off, g_pairs, g_qoff = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (off, pairs, qoff))
        N.check(N.lib().mvr_feat_match(N.ptr(feats), int(feats.shape[1]), N.ptr(g_off), len(off) - 1,
                                       int(feats.shape[0]), N.ptr(g_pairs), N.ptr(g_qoff), P, Q, int(nq.max()),
                                       N.ptr(idx), N.ptr(dist2), N.stream()), "mvr_feat_match")
    return idx, dist2, qoff


def match_features(feats, off, pairs, mutual=True):
    """Feature matches of every pair: mvr_feat_match source -> target and, with `mutual`, target -> source, keeping a
    match (i, j) only where j's nearest source row is i again.  feats, off, pairs as feat_match, pairs being
    (source, target).  -> a list of P int64 [n_p,2] device tensors of (source row, target row) within their
    fragments, ascending in the source row."""
    off, pairs = _check_inputs("match_features", feats, off, pairs)
    if len(pairs) == 0:
        return []
    idx_st, _, qoff = feat_match(feats, off, pairs)
    dev = feats.device
    P = len(pairs)
    n_src = torch.from_numpy(np.diff(qoff)).to(dev)
    pair_of = torch.repeat_interleave(torch.arange(P, device=dev), n_src)
    src_row = torch.arange(int(qoff[-1]), device=dev) - torch.from_numpy(qoff[:-1]).to(dev)[pair_of]
    tgt_row = idx_st.to(torch.int64)
    keep = tgt_row >= 0
    if mutual:
        idx_ts, _, roff = feat_match(feats, off, pairs[:, ::-1])
        back = torch.full_like(tgt_row, -1)
        at = torch.from_numpy(roff[:-1]).to(dev)[pair_of] + tgt_row
        back[keep] = idx_ts.to(torch.int64)[at[keep]]
        keep = keep & (back == src_row)
    both = torch.stack([src_row[keep], tgt_row[keep]], 1)
    counts = torch.bincount(pair_of[keep], minlength=P).cpu().tolist() if P else []
    return list(torch.split(both, counts))


KEYPOINT_MATCH = ("keypoints", "all")


def _keypoint_arguments(name, keypoints, match, B=None):
    """The checks of `keypoints` and `match` that need no device -> None (no keypoints), True (detect with the
    defaults) or (rows, off): the dict of FragmentOverlap.iss_keypoints, its rows as given and its off as numpy"""
    if match not in KEYPOINT_MATCH:
        raise ValueError("%s: match must be one of %s, not %r" % (name, ", ".join(KEYPOINT_MATCH), match))
    if keypoints is None or keypoints is True:
        return keypoints
    if not isinstance(keypoints, dict) or "rows" not in keypoints or "off" not in keypoints:
        raise ValueError("%s: keypoints must be None, True or the dict of FragmentOverlap.iss_keypoints "
                         "(with 'rows' and 'off')" % name)
    rows = keypoints["rows"]
    if not torch.is_tensor(rows) or rows.dim() != 1 or rows.dtype != torch.int64:
        raise ValueError("%s: keypoints['rows'] must be an int64 [K] tensor" % name)
    off = np.asarray(keypoints["off"], dtype=np.int64).reshape(-1)
    if len(off) < 2 or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != rows.shape[0] or \
            (B is not None and len(off) != B + 1):
        raise ValueError("%s: keypoints['off'] must be the [B+1] prefix sums of the keypoints per fragment, ending at "
                         "K" % name)
    return rows, off


def keypoint_match_rows(matches, pairs, off, kp_rows, kp_off, match="keypoints"):
    """Matches among keypoints back to rows within their fragments.  matches: per pair an int64 [n,2] tensor of
    (source keypoint, target keypoint) within their fragments' keypoints (match 'keypoints') or of (source keypoint,
    target row within its fragment) ('all'); off, kp_off [B+1]: the prefix sums of the points and of the keypoints per
    fragment; kp_rows int64 [K]: the keypoints' rows of fo.xyz, ascending.  Works on any device, the CPU included.
    -> a list of int64 [n,2] tensors of (source row, target row) within their fragments, the input of
    correspondences; ascending in the source row where the input is."""
    if match not in KEYPOINT_MATCH:
        raise ValueError("keypoint_match_rows: match must be one of %s, not %r" % (", ".join(KEYPOINT_MATCH), match))
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    off, kp_off = np.asarray(off, dtype=np.int64), np.asarray(kp_off, dtype=np.int64)
    out = []
    for p, m in enumerate(matches):
        i, j = int(pairs[p, 0]), int(pairs[p, 1])
        src = kp_rows[int(kp_off[i]) + m[:, 0]] - int(off[i])
        tgt = m[:, 1] if match == "all" else kp_rows[int(kp_off[j]) + m[:, 1]] - int(off[j])
        out.append(torch.stack([src, tgt], 1))
    return out


def match_keypoints(feats, off, pairs, kp_rows, kp_off, mutual=True, match="keypoints"):
    """match_features on the keypoint rows of feats alone (no new kernel), mapped back by keypoint_match_rows.
    match 'keypoints': keypoints against keypoints, on feats[kp_rows] with kp_off as the fragments.  'all': the
    source's keypoints against all target points — the keypoint rows are appended to feats as fragments B..2B-1 and
    the pairs become (B + i, j); `mutual` then means that the target point's nearest source keypoint is that one.
    -> as match_features: rows within the points' fragments."""
    off, pairs = _check_inputs("match_keypoints", feats, off, pairs)
    kp_off = np.asarray(kp_off, dtype=np.int64).reshape(-1)
    B = len(off) - 1
    sub = feats[kp_rows]
    if match == "all":
        matches = match_features(torch.cat([feats, sub]), np.concatenate([off, off[-1] + kp_off[1:]]),
                                 pairs + np.array([B, 0], dtype=np.int64), mutual)
    else:
        matches = match_features(sub, kp_off, pairs, mutual)
    return keypoint_match_rows(matches, pairs, off, kp_rows, kp_off, match)


def _matches(name, fo, pairs, mutual, keypoints, match):
    """The matching step of register_fpfh / register_fgr -> (matches, n_keypoints [P,2] or None)"""
    if keypoints is None:
        return match_features(fo.fpfh, fo.off, pairs, mutual), None
    if keypoints is True:
        kp = fo.iss_keypoints()
        keypoints = kp["rows"], kp["off"]
    rows, kp_off = keypoints
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= fo.M):
        raise ValueError("%s: keypoints['rows'] holds a row outside [0, %d)" % (name, fo.M))
    rows = rows.to(fo.device)
    n_kp = np.diff(kp_off)[pairs].astype(np.int64).reshape(-1, 2)
    return match_keypoints(fo.fpfh, fo.off, pairs, rows, kp_off, mutual, match), n_kp


CHECKER_KEYS = ("ransac_n", "iters", "max_validation", "edge_sim", "check_dist", "normal_deg")


def register_fpfh(fo, pairs, mutual=True, seed=0, ransac_n=RANSAC_N, max_dist=RANSAC_DIST, iters=RANSAC_ITERS,
                  checkers=False, keypoints=None, match="keypoints"):
    """Coarse registration of every pair of `fo` (a lib.overlap.FragmentOverlap after compute_fpfh()) from its FPFH
    matches: match_features, then lib.utils.run_ransac_batch over the matched points (its defaults: 4-point
    hypotheses, inliers within 0.05, 2500 iterations, draws keyed by `seed`).  pairs [P,2] (source, target).
    -> dict of numpy T fp64 [P,4,4] (x_target ~ T x_source; identity where a pair has fewer than ransac_n matches or
    no hypothesis has an inlier), fitness, rmse fp64 [P] (over the matches), n_matches int64 [P].
    checkers: True, or a dict overriding some of CHECKER_KEYS, runs lib.utils.run_ransac_checked_batch instead with
    its defaults (3-point samples, 100000 iterations of which at most 2500 are scored, the edge-length checker at
    0.9 and the distance checker at max_dist; `ransac_n` and `iters` above are then not used); 'normal_deg' adds the
    normal checker on fo.normals.  The dict then also holds n_pass and n_valid int32 [P].
    keypoints (None: every point is matched, the path as it was): True detects with fo.iss_keypoints(), a dict as that
    method returns is used as it is.  match 'keypoints' matches keypoints against keypoints, 'all' the source's
    keypoints against all target points (match_keypoints); n_matches counts what was matched and the dict also holds
    n_keypoints int64 [P,2] (source, target).  Everything after the matching is untouched."""
    if getattr(fo, "fpfh", None) is None:
        raise ValueError("register_fpfh: needs fo.fpfh (call fo.compute_fpfh())")
    if checkers is not False and checkers is not True:
        if not isinstance(checkers, dict) or set(checkers) - set(CHECKER_KEYS):
            raise ValueError("register_fpfh: checkers is a bool or a dict with keys among %s" % (CHECKER_KEYS,))
    keypoints = _keypoint_arguments("register_fpfh", keypoints, match, fo.B)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    matches, n_kp = _matches("register_fpfh", fo, pairs, mutual, keypoints, match)
    extra = {} if n_kp is None else {"n_keypoints": n_kp}
    P = len(pairs)
    counts = np.array([len(m) for m in matches], dtype=np.int64)
    xyz_s, xyz_t = correspondences(fo, pairs, matches)
    if checkers is not False:
        opts = dict(checkers) if isinstance(checkers, dict) else {}
        if P == 0:
            return {"T": np.zeros((0, 4, 4)), "fitness": np.zeros(0), "rmse": np.zeros(0), "n_matches": counts,
                    "n_pass": np.zeros(0, np.int32), "n_valid": np.zeros(0, np.int32), **extra}
        if opts.get("normal_deg") is not None:
            if fo.normals is None:
                raise ValueError("register_fpfh: the normal checker needs fo.normals")
            opts["normals_i"], opts["normals_j"] = correspondences(fo, pairs, matches, fo.normals)
        out = run_ransac_checked_batch(xyz_s, xyz_t, counts, seed=seed, max_dist=max_dist, device=fo.device, **opts)
        return {"T": out["T"], "fitness": out["fitness"], "rmse": out["rmse"], "n_matches": counts,
                "n_pass": out["n_pass"], "n_valid": out["n_valid"], **extra}
    if P == 0:
        return {"T": np.zeros((0, 4, 4)), "fitness": np.zeros(0), "rmse": np.zeros(0), "n_matches": counts, **extra}
    T, fit, rmse, _ = run_ransac_batch(xyz_s, xyz_t, counts, seed=seed, ransac_n=ransac_n, max_dist=max_dist,
                                       iters=iters, device=fo.device, return_all=True)
    return {"T": T, "fitness": fit, "rmse": rmse, "n_matches": counts, **extra}


def register_fgr(fo, pairs, mutual=True, seed=0, keypoints=None, match="keypoints", **fgr_options):
    """register_fpfh with Fast Global Registration (lib.utils.run_fgr_batch, csrc/fgr.hip mvr_fgr) in place of RANSAC:
    match_features, correspondences, then the graduated non-convexity over each pair's matches; fgr_options are
    run_fgr_batch's (max_dist, iters, division_factor, tuple_test, tuple_scale, max_tuples, tuple_factor), `seed`
    keys the tuple filter's draws.  No hypotheses are sampled, so it needs matches whose inlier share is tens of
    percent (FCGF descriptors' mutual matches, near-complete overlap); on FPFH matches of partly overlapping
    fragments the checked RANSAC of register_fpfh stays the choice.
    -> register_fpfh's keys (T, fitness, rmse, n_matches) plus n_used, n_tuples and status int32 [P]; pairs without
    matches get the identity (status 1).  keypoints, match: as register_fpfh (n_keypoints is added with them)."""
    if getattr(fo, "fpfh", None) is None:
        raise ValueError("register_fgr: needs fo.fpfh (call fo.compute_fpfh())")
    if set(fgr_options) & {"counts", "device", "return_trace"}:
        raise ValueError("register_fgr: counts, device and return_trace are not options")
    keypoints = _keypoint_arguments("register_fgr", keypoints, match, fo.B)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    matches, n_kp = _matches("register_fgr", fo, pairs, mutual, keypoints, match)
    extra = {} if n_kp is None else {"n_keypoints": n_kp}
    counts = np.array([len(m) for m in matches], dtype=np.int64)
    xyz_s, xyz_t = correspondences(fo, pairs, matches)
    if len(pairs) == 0:
        return {"T": np.zeros((0, 4, 4)), "fitness": np.zeros(0), "rmse": np.zeros(0), "n_matches": counts,
                "n_used": np.zeros(0, np.int32), "n_tuples": np.zeros(0, np.int32), "status": np.zeros(0, np.int32),
                **extra}
    out = run_fgr_batch(xyz_s, xyz_t, counts, seed=seed, device=fo.device, **fgr_options)
    return {"T": out["T"], "fitness": out["fitness"], "rmse": out["rmse"], "n_matches": counts,
            "n_used": out["n_used"], "n_tuples": out["n_tuples"], "status": out["status"], **extra}


def correspondences(fo, pairs, matches, rows=None):
    """The matched points of every pair, padded to the longest list: (source xyz, target xyz) fp64 [P,n,3] on the
    device, rows beyond a pair's count zero (the input of lib.utils.run_ransac_batch with counts).  rows: another
    fp64 [M,3] tensor in the row order of fo.xyz to gather instead (fo.normals)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P = len(pairs)
    rows = fo.xyz if rows is None else rows
    n = max([len(m) for m in matches] + [1])
    xyz_s = torch.zeros(P, n, 3, dtype=torch.float64, device=fo.device)
    xyz_t = torch.zeros(P, n, 3, dtype=torch.float64, device=fo.device)
    for p, m in enumerate(matches):
        xyz_s[p, :len(m)] = rows[int(fo.off[pairs[p, 0]]) + m[:, 0]]
        xyz_t[p, :len(m)] = rows[int(fo.off[pairs[p, 1]]) + m[:, 1]]
    return xyz_s, xyz_t
