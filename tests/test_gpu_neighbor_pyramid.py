"""geometry.neighbor_pyramid on an MI355X against postprocess.neighbor_pyramid, bit for bit: level points (the device voxel grid),
lengths, the three kinds of tables and their counts.  Run with `-m gpu`.  The pyramid strings together kernels that have their
own tests (tests/test_gpu_voxel_grid.py, tests/test_gpu_radius_pairs.py, tests/test_gpu_radius_neighbors.py); what is checked
here is the layer: which clouds meet in which pair, the index base and the pad of every table, float32 input, an empty cloud."""
import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

KINDS = ("neighbors", "subsampling", "upsampling")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def voxel_like(rng, n):
    """A 2.5 cm grid surface patch and the same patch with a 1 cm jitter: what a finished pair looks like at loader radii."""
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 0.025
    a = np.concatenate([g, 1.5 + 0.1 * np.sin(3 * g[:, :1])], 1) + rng.uniform(-0.004, 0.004, (n, 3))
    b = a + rng.normal(0, 0.01, (n, 3))
    return a, b[rng.permutation(n)]


def compare(points, lengths, device_lengths=False, **kw):
    from pointreggpt_amd import geometry as G
    want = PP.neighbor_pyramid(points, lengths, kw["num_stages"], kw["voxel_size"], kw["radius"], kw["neighbor_limits"])
    d_len = torch.tensor(list(lengths), dtype=torch.int64, device="cuda") if device_lengths else list(lengths)
    got = G.neighbor_pyramid(torch.from_numpy(np.ascontiguousarray(points)).cuda(), d_len, **kw)
    S = kw["num_stages"]
    assert sorted(got) == sorted(want) and sorted(got["counts"]) == sorted(KINDS)
    assert len(got["points"]) == len(got["lengths"]) == len(got["neighbors"]) == S
    assert len(got["subsampling"]) == len(got["upsampling"]) == S - 1
    for l in range(S):
        p, n = got["points"][l], got["lengths"][l]
        assert p.is_cuda and p.dtype == torch.float64 and n.is_cuda and n.dtype == torch.int64
        assert np.array_equal(n.cpu().numpy(), want["lengths"][l]), l
        assert p.shape == want["points"][l].shape and np.array_equal(bits(p.cpu().numpy()), bits(want["points"][l])), l
    for kind in KINDS:
        assert len(got[kind]) == len(want[kind]) == len(got["counts"][kind])
        for l, (t, c) in enumerate(zip(got[kind], got["counts"][kind])):
            assert t.is_cuda and t.dtype == torch.int32 and c.is_cuda and c.dtype == torch.int32
            assert t.shape == want[kind][l].shape and np.array_equal(t.cpu().numpy(), want[kind][l]), (kind, l)
            assert np.array_equal(c.cpu().numpy(), want["counts"][kind][l]), (kind, l)
    return want


def test_two_patches_three_stages():
    rng = np.random.default_rng(25)
    (a, _), (b, _) = voxel_like(rng, 1500), voxel_like(rng, 700)
    want = compare(np.concatenate([a, b]), [1500, 700], num_stages=3, voxel_size=0.025, radius=0.0625, neighbor_limits=(38, 36, 36))
    sizes = [len(p) for p in want["points"]]
    assert sizes[0] == 2200 and sizes[0] > sizes[1] > sizes[2] > 0
    assert (want["neighbors"][0] < 2200).any() and (want["neighbors"][0] == 2200).any()   # matches and pads


def test_truncating_limits_and_lengths_on_the_device():
    """Limits below the neighbour counts, so every table truncates; `lengths` as a device tensor."""
    rng = np.random.default_rng(26)
    (a, _), (b, _) = voxel_like(rng, 900), voxel_like(rng, 400)
    want = compare(np.concatenate([a, b]), [900, 400], device_lengths=True, num_stages=2, voxel_size=0.025, radius=0.0625,
                   neighbor_limits=(9, 5))
    for kind, limit in (("neighbors", 9), ("subsampling", 9), ("upsampling", 5)):
        assert (want["counts"][kind][0] > limit).any(), kind


def test_float32_input_is_widened():
    rng = np.random.default_rng(27)
    (a, _), (b, _) = voxel_like(rng, 700), voxel_like(rng, 513)
    pts32 = np.concatenate([a, b]).astype(np.float32)
    compare(pts32, [700, 513], num_stages=3, voxel_size=0.025, radius=0.0625, neighbor_limits=(38, 36, 36))


def test_four_clouds_one_of_them_empty():
    rng = np.random.default_rng(28)
    clouds = [voxel_like(rng, 600)[0], np.zeros((0, 3)), voxel_like(rng, 257)[1], voxel_like(rng, 64)[0] + 5.0]
    want = compare(np.concatenate(clouds), [len(c) for c in clouds], num_stages=3, voxel_size=0.025, radius=0.0625,
                   neighbor_limits=(20, 20, 20))
    assert all(n[1] == 0 for n in want["lengths"]) and all(n[0] > 0 and n[2] > 0 and n[3] > 0 for n in want["lengths"])
