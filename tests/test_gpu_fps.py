"""GPU farthest point sampling (csrc/fps.hip via lib.fps / Sampler('fps')) vs the numpy
restatement oracle/fps.py — indices bit-exact (parity unpinned: pointnet2_ops is not vendored)."""
import numpy as np
import pytest

from synth import synth_scene_fragments

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sizes,m", [([100, 257], 50), ([3000, 5000, 1024], 700), ([20000], 600), ([24000, 17000], 900),
                                    ([30000], 300), ([4096, 8192, 16384], 1000)])
def test_fps_matches_oracle(gpu, sizes, m):
    import torch
    from lib.fps import furthest_point_sample
    from oracle.fps import sample_fps
    r = np.random.RandomState(sum(sizes))
    xyz = np.concatenate([r.uniform(-2, 2, (n, 3)).astype(np.float32) for n in sizes])
    got = furthest_point_sample(torch.from_numpy(xyz).to(gpu), sizes, m).cpu().numpy()
    ref = sample_fps(xyz, sizes, m)
    np.testing.assert_array_equal(got, ref)


def test_sampler_fps_on_voxelised_fragments(gpu):
    import torch
    from lib.layers import Sampler
    from lib.sparse import voxelize
    from oracle.fps import sample_fps
    frags, _ = synth_scene_fragments(2, seed=3, n_pts=40000)
    coords, sel, counts, xyz = voxelize([torch.from_numpy(f) for f in frags], 0.025, gpu)
    F = torch.randn(xyz.shape[0], 32, device=gpu)
    sc, sf = Sampler("fps", 800)(xyz, F, torch.tensor(counts))
    idx = sample_fps(xyz.cpu().numpy(), counts, 800)
    np.testing.assert_array_equal(sc.cpu().numpy(), xyz.cpu().numpy()[idx])
    np.testing.assert_array_equal(sf.cpu().numpy(), F.cpu().numpy()[idx])


def test_fps_rejects_too_few_points(gpu):
    import torch
    from lib.fps import furthest_point_sample
    with pytest.raises(RuntimeError):
        furthest_point_sample(torch.zeros(10, 3, device=gpu), [10], 11)


def _fps_both(gpu, xyz, sizes, m):
    import torch
    from lib.fps import furthest_point_sample
    from oracle.fps import sample_fps
    got = furthest_point_sample(torch.from_numpy(xyz).to(gpu), sizes, m).cpu().numpy()
    assert got.shape == (len(sizes), m) and got.dtype == np.int64
    return got, sample_fps(xyz, sizes, m)


def _uniform(sizes, seed):
    r = np.random.RandomState(seed)
    return np.concatenate([r.uniform(-2, 2, (n, 3)).astype(np.float32) for n in sizes])


# the capacities of mvr_fps's kernel ladder (1024 threads x 4, 8, 16, 20, 24 points in registers; 1024 x 64 and
# 512 x 160 re-reading from L2) and the first size past each; 81,920 is the largest fragment
@pytest.mark.parametrize("n", [4096, 4097, 8192, 8193, 16384, 16385, 20480, 20481, 24576, 24577, 65536, 65537, 81920])
def test_fps_rung_edges(gpu, n):
    got, ref = _fps_both(gpu, _uniform([n], n), [n], 64)
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("n", [4096, 4097, 8192, 8193, 16384, 16385, 20480, 20481, 24576, 24577, 65536, 65537, 81920])
def test_fps_last_row_of_a_rung_edge_is_seen(gpu, n):
    """the fragment's last row is far outside the cloud, so it is the second draw: a kernel instance one point short
    of the fragment (a rung chosen too low) cannot pass, whatever the first 64 draws of the uniform cloud are"""
    xyz = _uniform([n], 7 * n)
    xyz[-1] = [40.0, -40.0, 40.0]
    got, ref = _fps_both(gpu, xyz, [n], 3)
    np.testing.assert_array_equal(got, ref)
    assert got[0, 0] == 0 and got[0, 1] == n - 1


def test_fps_rejects_a_fragment_past_the_largest_kernel(gpu):
    import torch
    from lib.fps import furthest_point_sample
    with pytest.raises(RuntimeError):
        furthest_point_sample(torch.zeros(81921, 3, device=gpu), [81921], 64)


@pytest.mark.parametrize("sizes,m", [([3, 70000, 1], 1), ([40, 70000], 40)])
def test_fps_small_fragment_in_a_large_batch(gpu, sizes, m):
    """the batch's largest fragment selects the L2 re-read kernel (512 threads x 160 points); the small fragments ride
    in it with nearly every slot absent.  m == n for the 40-point fragment: all of its rows, each once."""
    got, ref = _fps_both(gpu, _uniform(sizes, 5), sizes, m)
    np.testing.assert_array_equal(got, ref)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for b, n in enumerate(sizes):
        assert got[b, 0] == off[b] and (got[b] >= off[b]).all() and (got[b] < off[b + 1]).all()
        if m == n:
            np.testing.assert_array_equal(np.sort(got[b]), np.arange(off[b], off[b + 1]))


@pytest.mark.parametrize("n", [1, 64, 4096, 4097])
def test_fps_draws_every_point_when_m_equals_n(gpu, n):
    got, ref = _fps_both(gpu, _uniform([n], 1000 + n), [n], n)
    np.testing.assert_array_equal(np.sort(got[0]), np.arange(n))      # a permutation of the fragment's rows
    np.testing.assert_array_equal(got, ref)


def test_fps_identical_points(gpu):
    """every distance is 0 from the first step on: the lowest index wins each time, as numpy's argmax"""
    xyz = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (5000, 1))
    got, ref = _fps_both(gpu, xyz, [5000], 10)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got, np.zeros((1, 10), np.int64))


def test_fps_ties_take_the_lowest_index(gpu):
    """exact distance ties (duplicated points, a lattice): the first maximum in fragment order wins, as numpy's
    argmax in the oracle"""
    import torch
    from lib.fps import furthest_point_sample
    from oracle.fps import sample_fps
    g = np.stack(np.meshgrid(*[np.arange(12, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    xyz = np.concatenate([g, g[::-1], g[:500]])            # every point at least twice
    sizes = [len(xyz)]
    got = furthest_point_sample(torch.from_numpy(xyz).to(gpu), sizes, 700).cpu().numpy()
    np.testing.assert_array_equal(got, sample_fps(xyz, sizes, 700))
