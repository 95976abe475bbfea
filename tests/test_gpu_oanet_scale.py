"""OANet + Procrustes at the batch sizes the benchmark runs in ONE forward — 435 pairs (the 30-fragment scene), 1,225
(the 50-fragment scene) and 1,700 — against the float64 oracle on sampled pairs and, bit for bit on every pair, against
the same pairs run 32 at a time (the path tests/test_gpu_oanet.py pins to the reference's fixtures).

Why these sizes: csrc/oanet.hip plan() lays X11 out as [P][2C][Np] and XA, T1 and the returned activation as
[P][C][Np] with C = 128, Np = round32(5000) = 5024: 5,144,576 and 2,572,288 bytes per pair.  The point convs and the
fused attention kernels address a pair through a 64-bit pair base plus 32-bit offsets, partition (pair, tile) ranges
over a persistent grid and deal pairs to workgroups in octets — all functions of P that no 32-pair test reaches.
Largest offsets covered (last pair's slab end):

    P       X11 bytes / elements              XA, T1, latent bytes / elements       block workspace (measured)
    435     2,237,890,560 /   559,472,640     1,118,945,280 /   279,736,320          5,371,379,200 B
    1225    6,302,105,600 / 1,575,526,400     3,151,052,800 /   787,763,200         15,123,423,744 B
    1700    8,745,779,200 / 2,186,444,800     4,372,889,600 / 1,093,222,400         20,986,994,688 B

so 435 crosses 2^31 bytes in X11 (pairs 417 | 418), 1225 crosses 2^32 bytes in X11 and 2^31 bytes in XA / T1 (834 | 835),
and 1700 crosses 2^31 ELEMENTS in X11 and 2^32 bytes in XA / T1 (1669 | 1670).  The workspace column is
mvr_oan_block_workspace_bytes(128, 500, 8, P, 5000); at P = 1700 the forward needs it plus 5,054,378,800 B of inputs and
outputs (26.04 GB), and the P = 1700 case skips only when less than 1.5 x that is free.

Inputs: the well-conditioned network and correspondences of tests/golden/oanet_full_train_strict.npz (weights seed 19, correspondences seed 40
with 20-50 % inliers; synth_correspondences draws pair after pair from one stream, so P pairs extend the fixture's 32).
The oracle's own fp32 result lies within 5e-6 of its fp64 result on every sampled pair (measured on the CPU: eval pairs
{0, 1, 217, 433, 434} and the train group 416..434 of P = 435; eval pairs {834, 835, 1222, 1224, 1669, 1670, 1697,
1699} at most 9.8e-7 in R and 3.4e-6 in t; the train group 1216..1224 of P = 1225 at most 8.2e-7 / 4.5e-6), every pair
has >= 3,289 positive logits (the zero-row guard is idle) and at most 2 scores per pair lie within 1e-4 of 0.5.
"""
import json
import os
import time

import numpy as np
import pytest

from conftest import GOLDEN
from synth import synth_state, synth_correspondences

pytestmark = pytest.mark.gpu

C, K, N = 128, 500, 5000          # channels, clusters, correspondences (RegBlock.yaml)
NP = (N + 31) // 32 * 32          # padded point row (csrc/oanet.hip plan(): round32)
X11_SLAB = 2 * C * NP * 4         # bytes of one pair in X11 [P][2C][Np]
XA_SLAB = C * NP * 4              # ... in XA, T1 and the returned activation [P][C][Np]
BATCH = 32                        # the loader batch (scripts/benchmark_pairwise_registration.py)
WEIGHTS_SEED, XS_SEED, INLIERS = 19, 40, (0.2, 0.5)
P_MAX = 1700
KEYS = ("logits", "scores", "rot_est", "trans_est")


def _crossings():
    """(pair that holds the boundary, first pair past it) for every power-of-two limit a batch up to P_MAX crosses"""
    out = []
    for limit, slab in ((1 << 31, X11_SLAB), (1 << 32, X11_SLAB), (4 << 31, X11_SLAB),   # bytes, bytes, elements
                        (1 << 31, XA_SLAB), (1 << 32, XA_SLAB)):
        p = limit // slab
        out += [p, p + 1]
    return sorted(set(out))


def sampled(P):
    """S(P): the first two pairs, the pairs on either side of each crossing, and two pairs of the ragged last octet /
    32-group"""
    assert P % 8 and P % BATCH, P
    return sorted(p for p in set([0, 1, P - 3, P - 1] + _crossings()) if 0 <= p < P)


def test_sampled_pairs_sit_on_the_layout_boundaries(gpu):
    """a change of the activation layout must move these on purpose, not quietly"""
    assert (NP, X11_SLAB, XA_SLAB) == (5024, 5144576, 2572288)
    assert _crossings() == [417, 418, 834, 835, 1669, 1670]
    assert sampled(435) == [0, 1, 417, 418, 432, 434]
    assert sampled(1225) == [0, 1, 417, 418, 834, 835, 1222, 1224]
    assert sampled(1700) == [0, 1, 417, 418, 834, 835, 1669, 1670, 1697, 1699]


# ---------------------------------------------------------------------------------------------- shared inputs
_cache = {}


def _state():
    if "state" not in _cache:
        with open(os.path.join(GOLDEN, "oanet_keys.json")) as f:
            _cache["state"] = synth_state(json.load(f)["full"], seed=WEIGHTS_SEED)
    return _cache["state"]


def _xs(P):
    """synth_correspondences(P, 5000, seed 40, inliers 20-50 %): drawn once at the largest P (the generator is
    sequential in the pair index: checked on the first pairs), read-only"""
    if "xs" not in _cache:
        xs, _, _ = synth_correspondences(P_MAX, N, seed=XS_SEED, inlier_lo=INLIERS[0], inlier_hi=INLIERS[1])
        head, _, _ = synth_correspondences(2, N, seed=XS_SEED, inlier_lo=INLIERS[0], inlier_hi=INLIERS[1])
        assert np.array_equal(head, xs[:2])
        _cache["xs"] = xs
    return _cache["xs"][:P]


def _oracle_eval(pairs):
    """float64 oracle of single pairs in eval mode (pairs are independent there while the guard is idle, which the
    caller asserts): each pair is computed once for all the batch sizes that sample it"""
    from oracle.oanet import oanet_forward
    memo = _cache.setdefault("oracle_eval", {})
    todo = [p for p in pairs if p not in memo]
    if todo:
        o = oanet_forward(_state(), _xs(P_MAX)[todo], dtype=np.float64)
        for j, p in enumerate(todo):
            memo[p] = {k: [o[k][i][j] for i in range(2)] for k in KEYS}
    return {k: [np.stack([memo[p][k][i] for p in pairs]) for i in range(2)] for k in KEYS}


def _net(gpu, train):
    import torch
    import bench
    from lib.filtering.oanet import OANet
    net = OANet(bench.oanet_cfg())
    st = _state()
    assert set(net.state_dict()) == set(st)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    return net.to(gpu).train(train)


def _forward_bytes(P):
    """device bytes of one forward over P pairs: the block workspace, and the input / output tensors of
    lib/filtering/oanet.py forward() (xs, the channel-major input, the returned activation, per block logits, scores,
    residuals, R, t, status, and the guard counts)"""
    from lib import _native as NV
    ws = max(NV.lib().mvr_oan_block_workspace_bytes(C, K, cin, P, N) for cin in (6, 8))
    io = 4 * P * (N * 6 + 8 * NP + C * NP + 2 * (3 * N + 9 + 3 + 1) + 1)
    return ws, io


@pytest.fixture(scope="module", autouse=True)
def _release_workspace():
    """the 21 GB workspace of the largest forward is not kept for the rest of the session"""
    yield
    import torch
    from lib import _native as NV
    _cache.clear()
    NV._ws_cache.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _timed(fn):
    """fn() with its device time (ms, events on the current stream) and wall time (s)"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.time()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1), time.time() - t0


def _whole_forward(net, X):
    import torch
    with torch.no_grad():
        return net({"xs": X})


def _guard_idle(out):
    """every pair has a positive logit in both blocks (logits, not scores: a fired guard adds 1 / N to every score)"""
    return all(bool((out["logits"][i] > 0).any(dim=1).all()) for i in range(2))


def _assert_equals_chunks(net, X, whole, chunk_forward):
    """`whole` bit for bit against chunk_forward(X[b0:b0 + 32]) of every consecutive 32-pair chunk: logits, scores,
    R, t of both blocks and the returned activation, on every pair"""
    import torch
    P = X.shape[0]
    bad = []
    for b0 in range(0, P, BATCH):
        part = chunk_forward(net, X[b0:b0 + BATCH])
        b1 = min(P, b0 + BATCH)
        for i in range(2):
            for k in KEYS:
                if not torch.equal(whole[k][i][b0:b1], part[k][i]):
                    bad.append((b0, k, i))
        if not torch.equal(whole["latent features"][b0:b1], part["latent features"]):
            bad.append((b0, "latent features"))
    assert not bad, "whole batch != 32-pair chunks at (first pair of chunk, output, block): %s" % bad[:12]


def _assert_matches_oracle(out, rows, ref, tag):
    """rows of `out` against the float64 oracle `ref` (same order): R, t within 1e-4 (the bound of
    test_oanet_full_train_strict_golden), logits within 2e-3 + 1e-4 relative, masks equal where the oracle's score is
    at least 1e-4 from 0.5, and at most 16 scores per block that close (a condition on the input, <= 2 per pair in the
    oracle alone).  Returns the largest R and t distances."""
    import torch
    rows = torch.as_tensor(np.asarray(rows), device=out["scores"][0].device)
    worst = [0.0, 0.0]
    for i in range(2):
        sc = out["scores"][i][rows].cpu().numpy()
        rsc = ref["scores"][i]
        near = np.abs(rsc - 0.5) < 1e-4
        assert near.sum() <= 16, (tag, i, int(near.sum()))
        for j, (k, tol) in enumerate((("rot_est", 1e-4), ("trans_est", 1e-4))):
            d = np.abs(out[k][i][rows].cpu().numpy() - ref[k][i]).reshape(len(rows), -1).max(1)
            worst[j] = max(worst[j], float(d.max()))
            print("%s block %d %s: max |gpu - fp64 oracle| per sampled pair %s" % (tag, i, k, np.array2string(d, precision=2)))
            assert (d <= tol).all(), (tag, i, k, d)
        np.testing.assert_allclose(out["logits"][i][rows].cpu().numpy(), ref["logits"][i], atol=2e-3, rtol=1e-4)
        assert np.array_equal((sc > 0.5)[~near], (rsc > 0.5)[~near]), (tag, i)
    return worst


# ---------------------------------------------------------------------------------------------- test 1: eval
@pytest.mark.parametrize("P", [435, 1225, 1700])
def test_eval_whole_batch_equals_chunks_and_oracle(gpu, P):
    """Eval mode, guard_group = 0 (the scene benchmark's configuration), one forward over P pairs:
    (a) the zero-row guard is idle; (b) every output of every pair is bit-identical to the same pairs run in
    consecutive chunks of 32; (c) the pairs S(P) are within the strict bound of the float64 oracle.

    Measured on an MI355X (whole forward device time; test wall time incl. the CPU oracle; largest distance from the
    fp64 oracle over S(P) in R / t):
        P = 435:   52 ms + 14 chunk forwards and compares 135 ms; 2.8 s; 8.7e-7 / 6.8e-7
        P = 1225:  87 ms + 39 chunk forwards and compares 156 ms; 1.3 s; 5.7e-7 / 6.8e-7
        P = 1700: 610 ms (the first call at this size: it allocates the 21 GB workspace) + 54 chunks 235 ms; 5.0 s;
                  1.5e-6 / 6.8e-7; not skipped (288 GB device)"""
    import torch
    ws, io = _forward_bytes(P)
    if P == P_MAX:
        free = torch.cuda.mem_get_info(gpu)[0]
        if free < 1.5 * (ws + io):
            pytest.skip("P = 1700 needs %d B of workspace + %d B of inputs and outputs; 1.5 x that is not free (%d B)"
                        % (ws, io, free))
    t0 = time.time()
    S = sampled(P)
    ref = _oracle_eval(S)
    t_oracle = time.time() - t0
    for i in range(2):   # the oracle's own guard is idle too: its pairs are independent, as _oracle_eval assumes
        assert (ref["logits"][i] > 0).any(axis=1).all()
    net = _net(gpu, train=False)
    assert net.guard_group == 0 and net.bn_group == 0
    X = torch.from_numpy(_xs(P)).unsqueeze(1).to(gpu)
    whole, ms, _ = _timed(lambda: _whole_forward(net, X))
    assert _guard_idle(whole)                                        # (a)
    _, ms_chunks, _ = _timed(lambda: _assert_equals_chunks(net, X, whole, _whole_forward))   # (b)
    worst = _assert_matches_oracle(whole, S, ref, "eval P=%d" % P)   # (c)
    assert whole["gradient_flag"] == False                           # noqa: E712 (a DeviceFlag)
    print("eval P=%d: whole forward %.1f ms, %d chunk forwards + compares %.1f ms, oracle (new pairs) %.1f s, "
          "workspace %d B + io %d B, max dR %.2e dt %.2e, wall %.1f s"
          % (P, ms, -(-P // BATCH), ms_chunks, t_oracle, ws, io, worst[0], worst[1], time.time() - t0))


# ---------------------------------------------------------------------------------------------- test 2: train
@pytest.mark.parametrize("P", [435, 1225])
def test_train_grouped_equals_batches_and_oracle(gpu, P):
    """Train mode with bn_group = guard_group = 32 (bench.PrecomputedWorkload: the reference benchmark's 32-pair loader
    batches side by side in one forward): (a) bit-identical to one forward per loader batch with bn_group =
    guard_group = 0, every batch, every pair; (b) the last, ragged group (19 pairs at P = 435, 9 at P = 1225) within
    the strict bound of the float64 oracle run on that batch in train mode.

    Measured on an MI355X (grouped forward device time; wall time, nearly all of it the float64 oracle on the CPU;
    largest distance from the oracle over the last group in R / t):
        P = 435:  34 ms + 14 batch forwards and compares 67 ms; 6.7 s; 5.5e-7 / 5.0e-7
        P = 1225: 88 ms + 39 batch forwards and compares 188 ms; 3.7 s; 3.5e-7 / 4.5e-7"""
    import torch
    from oracle.oanet import oanet_forward
    t0 = time.time()
    xs = _xs(P)
    g0 = (P - 1) // BATCH * BATCH
    assert P - g0 == {435: 19, 1225: 9}[P]
    o = oanet_forward(_state(), xs[g0:P], train=True, dtype=np.float64)
    ref = {k: [np.asarray(o[k][i]) for i in range(2)] for k in KEYS}
    t_oracle = time.time() - t0
    net = _net(gpu, train=True)
    X = torch.from_numpy(xs).unsqueeze(1).to(gpu)
    net.bn_group = net.guard_group = BATCH
    whole, ms, _ = _timed(lambda: _whole_forward(net, X))
    assert _guard_idle(whole)

    def per_batch(n, x):
        n.bn_group = n.guard_group = 0
        return _whole_forward(n, x)
    _, ms_chunks, _ = _timed(lambda: _assert_equals_chunks(net, X, whole, per_batch))               # (a)
    worst = _assert_matches_oracle(whole, list(range(g0, P)), ref, "train P=%d" % P)                 # (b)
    assert whole["gradient_flag"] == False                                                           # noqa: E712
    print("train P=%d: grouped forward %.1f ms, %d batch forwards + compares %.1f ms, oracle %.1f s, max dR %.2e "
          "dt %.2e, wall %.1f s" % (P, ms, -(-P // BATCH), ms_chunks, t_oracle, worst[0], worst[1], time.time() - t0))


# ---------------------------------------------------------------------------------------------- test 3: the scene
@pytest.mark.parametrize("n_frag", [30, 50])
def test_scene_filtering_whole_equals_chunks(gpu, n_frag):
    """The benchmark's own scene (bench.SceneWorkload: FCGF -> sampler -> feature NN over all 435 / 1,225 pairs ->
    OANet + Procrustes, seed-7 weights): (a) the feature NN's matches of the pairs S(P) against oracle/soft_nn.py fed
    the GPU's sampled descriptors and coordinates (2e-5, the bound of test_pairwise_reg_end_to_end_vs_oracle);
    (b) filter_correspondences over all pairs bit-identical to chunks of 32.  The zero-row guard is NOT idle on these
    scenes (143 of 435 and 435 of 1,225 pairs have no positive logit in block 0 with this random network), so both
    sides run with guard_group = 32: the guard's scope is the 32-pair chunk in the whole forward as in the chunked
    one.  No R / t bound against the oracle here: this random network is not known to be well conditioned (tests 1
    and 2 carry that bound).

    Measured on an MI355X (feature-NN distance from the oracle; filtering device time; wall time incl. building the
    scene):
        30 fragments: 2.5e-6; 35 ms + 14 chunk forwards and compares 134 ms; 5.4 s
        50 fragments: 1.4e-6; 144 ms + 39 chunk forwards and compares 153 ms; 7.1 s"""
    import torch
    import bench
    from oracle.soft_nn import soft_nn, pair_index
    t0 = time.time()
    wl = bench.SceneWorkload(gpu, 0, n_frag=n_frag)
    P = wl.pairs
    assert P == {30: 435, 50: 1225}[n_frag]
    model = wl.model
    got = {}
    inner = model.match_samples

    def match_samples(data, xyz_b, f_b, F0, F1):   # the sampled (coordinates, descriptors) describe() matches
        got["xyz"], got["f"] = xyz_b, f_b
        return inner(data, xyz_b, f_b, F0, F1)
    model.match_samples = match_samples
    try:
        with torch.no_grad():
            fin = wl.describe()
    finally:
        del model.match_samples
    xs = fin["xs"]
    assert tuple(xs.shape) == (P, 1, N, 6)
    # (a)
    S = sampled(P)
    pi = pair_index(n_frag)[S]
    Xs, Fs = got["xyz"].cpu().numpy(), got["f"].cpu().numpy()
    xc = soft_nn(Fs[pi[:, 0]], Fs[pi[:, 1]], Xs[pi[:, 1]], "soft", st=False, temp=0.3)
    mine = xs[S, 0].cpu().numpy()
    np.testing.assert_array_equal(mine[..., :3], Xs[pi[:, 0]])
    d_nn = float(np.abs(mine[..., 3:] - xc).max())
    print("scene n_frag=%d: max |feature-NN match - oracle| over S(P) %.2e" % (n_frag, d_nn))
    np.testing.assert_allclose(mine[..., 3:], xc, atol=2e-5)
    # (b)
    filt = model.filtering_module
    assert not filt.training and filt.guard_group == 0 and filt.guard_sync is None
    filt.guard_group = BATCH   # the guard is NOT idle on this scene (docstring): its scope is the 32-pair chunk

    def run(m, x):
        with torch.no_grad():
            return m.filter_correspondences({"xs": x})
    whole, ms, _ = _timed(lambda: run(model, xs))
    zero_rows = [int((~(whole["logits"][i] > 0).any(dim=1)).sum()) for i in range(2)]
    _, ms_chunks, _ = _timed(lambda: _assert_equals_chunks(model, xs, whole, run))
    print("scene n_frag=%d (%d pairs): filtering %.1f ms, %d chunk forwards + compares %.1f ms, pairs without a "
          "positive logit per block %s, wall %.1f s" % (n_frag, P, ms, -(-P // BATCH), ms_chunks, zero_rows,
                                                         time.time() - t0))
