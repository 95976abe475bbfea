"""Host-side checks of lib.multiview._scene_batch, the marshaller synchronize and optimize_pose_graph share, on CPU
tensors (they stay on the host where there is no device): three ragged scenes given as per-scene lists, as hand-padded
arrays with n_frags / n_edges, and one of them alone come out as the same padded tensors, for both entries' field
sets."""
import numpy as np
import pytest
import torch

FRAGS, EDGES = (1, 2, 3), (0, 1, 3)


def _scenes(dtype=np.float64):
    rng = np.random.default_rng(31)
    out = []
    for n, e in zip(FRAGS, EDGES):
        out.append({"R": rng.standard_normal((n, 3, 3)).astype(dtype), "t": rng.standard_normal((n, 3)).astype(dtype),
                    "R_pair": rng.standard_normal((e, 3, 3)).astype(dtype),
                    "t_pair": rng.standard_normal((e, 3)).astype(dtype),
                    "pairs": rng.integers(0, n, (e, 2)), "weights": rng.uniform(0.5, 1.5, e).astype(dtype),
                    "info": rng.standard_normal((e, 6, 6)).astype(dtype), "uncertain": rng.integers(0, 3, e)})
    return out


def _padded(scs, key):
    tail = scs[-1][key].shape[1:]
    n = max(len(s[key]) for s in scs)
    out = np.zeros((len(scs), n) + tail, scs[-1][key].dtype)
    for k, s in enumerate(scs):
        out[k, :len(s[key])] = s[key]
    return out


def _batch(which, get, n_frags=None, n_edges=None, weights=True, wrap=lambda x: x):
    """_scene_batch with synchronize's fields ("sync") or optimize_pose_graph's ("pg"); get(key) -> the argument"""
    from lib import multiview as M
    edge = M._edge_fields(wrap(get("R_pair")), wrap(get("t_pair")), wrap(get("pairs")),
                          wrap(get("weights")) if weights else None)
    if which == "sync":
        return M._scene_batch("synchronize", edge, (), n_frags, n_edges, 0, edge[0][1])
    edge += (("info", wrap(get("info")), (36,), torch.float64, False),
             ("uncertain flag", wrap(get("uncertain")) if weights else None, (), M.FLAG, True))
    frag = (("R", wrap(get("R")), (3, 3), torch.float64, False), ("t", wrap(get("t")), (3,), torch.float64, False))
    return M._scene_batch("optimize_pose_graph", edge, frag, n_frags, n_edges, 0, frag[0][1])


def _same(a, b, rows=slice(None)):
    assert a.x.keys() == b.x.keys()
    for k in a.x:
        assert (a.x[k] is None) == (b.x[k] is None), k
        if a.x[k] is not None:
            assert a.x[k][rows].dtype == b.x[k].dtype and torch.equal(a.x[k][rows], b.x[k]), k


@pytest.mark.parametrize("which", ["sync", "pg"])
def test_the_three_forms_give_the_same_tensors(which):
    scs = _scenes()
    lists = _batch(which, lambda k: [s[k] for s in scs], n_frags=list(FRAGS) if which == "sync" else None)
    padded = _batch(which, lambda k: _padded(scs, k), n_frags=list(FRAGS), n_edges=list(EDGES))
    _same(lists, padded)
    for b in (lists, padded):
        assert (b.S, b.Fmax, b.Emax, b.nf, b.ne) == (3, 3, 3, list(FRAGS), list(EDGES))
        assert b.n_f.tolist() == list(FRAGS) and b.n_e.tolist() == list(EDGES) and b.n_f.dtype == torch.int32
        assert all(v.is_contiguous() for v in b.x.values())
        assert b.x["R_pair"].shape == (3, 3, 3, 3) and b.x["pair"].dtype == torch.int32
        assert b.x["weight"].shape == (3, 3) and b.x["weight"].dtype == torch.float64
    if which == "pg":
        assert lists.x["info"].shape == (3, 3, 36) and lists.x["uncertain flag"].dtype == torch.int32
        assert lists.x["uncertain flag"].tolist() == (_padded(scs, "uncertain") != 0).astype(int).tolist()
    # the padding is zero, whatever the caller's padded arrays hold there
    assert not lists.x["R_pair"][0].any() and not lists.x["R_pair"][1, 1:].any()
    # one scene alone: the same rows behind a leading [1]
    alone = _batch(which, lambda k: scs[2][k], n_frags=3 if which == "sync" else None)
    assert (alone.S, alone.Fmax, alone.Emax, alone.nf, alone.ne) == (1, 3, 3, [3], [3])
    _same(lists, alone, slice(2, 3))
    # t_pair [E,3,1] and info [E,36] are accepted
    col = _batch(which, lambda k: scs[2][k][..., None] if k == "t_pair" else scs[2][k].reshape(3, -1)
                 if k == "info" else scs[2][k], n_frags=3 if which == "sync" else None)
    _same(alone, col)


@pytest.mark.parametrize("which", ["sync", "pg"])
def test_fp32_comes_out_fp64_and_an_absent_field_stays_none(which):
    scs = _scenes(np.float32)
    nf = list(FRAGS) if which == "sync" else None
    b = _batch(which, lambda k: [s[k] for s in scs], n_frags=nf, weights=False)
    assert b.x["weight"] is None and b.x["R_pair"].dtype == torch.float64
    assert torch.equal(b.x["R_pair"][2].cpu(), torch.from_numpy(scs[2]["R_pair"].astype(np.float64)))
    if which == "pg":
        assert b.x["uncertain flag"] is None and b.x["R"].dtype == torch.float64 and b.x["info"].dtype == torch.float64


@pytest.mark.parametrize("which", ["sync", "pg"])
def test_finish_hands_back_what_was_given(which):
    scs = _scenes()
    nf = list(FRAGS) if which == "sync" else None
    out = {"R": torch.arange(27.0).reshape(3, 3, 3), "status": torch.tensor([1, 2, 3], dtype=torch.int32)}
    got = _batch(which, lambda k: [s[k] for s in scs], n_frags=nf).finish(out)
    assert isinstance(got["R"], np.ndarray) and got["R"].shape == (3, 3, 3) and got["status"].tolist() == [1, 2, 3]
    got = _batch(which, lambda k: [s[k] for s in scs], n_frags=nf, wrap=lambda v: [torch.as_tensor(x) for x in v])
    got = got.finish(out)
    assert torch.is_tensor(got["R"]) and got["R"].device.type == "cpu" and got["R"].shape == (3, 3, 3)
    one = {k: v[:1] for k, v in out.items()}
    got = _batch(which, lambda k: scs[2][k], n_frags=3 if which == "sync" else None).finish(one)
    assert isinstance(got["R"], np.ndarray) and got["R"].shape == (3, 3) and got["status"].shape == () \
        and got["status"] == 1
    got = _batch(which, lambda k: scs[2][k], n_frags=3 if which == "sync" else None, wrap=torch.as_tensor).finish(one)
    assert torch.is_tensor(got["R"]) and got["R"].shape == (3, 3) and got["status"].dim() == 0
    got = _batch(which, lambda k: scs[2][k][None], n_frags=[3], wrap=torch.as_tensor).finish(one)
    assert torch.is_tensor(got["R"]) and got["R"].shape == (1, 3, 3)
