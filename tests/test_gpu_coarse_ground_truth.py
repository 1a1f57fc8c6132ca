"""geometry.coarse_ground_truth on an MI355X against postprocess.coarse_ground_truth, bit for bit.  Run with `-m gpu`.  The
kernels have their own tests (tests/test_gpu_patches.py); what is checked here is the layer on the pyramid: which level is fine
and which the nodes, which clouds form an item, the stack indices and the pad of every table, float32 input."""
import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

KW = dict(num_stages=3, voxel_size=0.025, radius=0.0625, neighbor_limits=(20, 20, 20))
LIMIT, RADIUS = 8, 0.05


def voxel_like(rng, n):
    """A 2.5 cm grid surface patch and the same patch with a 1 cm jitter: what a finished pair looks like at loader radii."""
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 0.025
    a = np.concatenate([g, 1.5 + 0.1 * np.sin(3 * g[:, :1])], 1) + rng.uniform(-0.004, 0.004, (n, 3))
    b = a + rng.normal(0, 0.01, (n, 3))
    return a, b[rng.permutation(n)][: n - n // 10]


@pytest.fixture(scope="module")
def pyramids():
    """Two items of ~600-row clouds in float32: the host pyramid (the reference, computed once) and the device pyramid."""
    from pointreggpt_amd import geometry as G
    rng = np.random.default_rng(31)
    clouds = [c for n in (620, 577) for c in voxel_like(rng, n)]
    pts32 = np.concatenate(clouds).astype(np.float32)
    lens = [len(c) for c in clouds]
    want = PP.neighbor_pyramid(pts32, lens, KW["num_stages"], KW["voxel_size"], KW["radius"], KW["neighbor_limits"])
    got = G.neighbor_pyramid(torch.from_numpy(pts32).cuda(), lens, **KW)
    return want, got


@pytest.mark.parametrize("fine_level", [0, 1, 2])
def test_coarse_ground_truth_equals_the_specification(pyramids, fine_level):
    from pointreggpt_amd import geometry as G
    host, dev = pyramids
    want = PP.coarse_ground_truth(host, fine_level=fine_level, limit=LIMIT, radius=RADIUS)
    got = G.coarse_ground_truth(dev, fine_level=fine_level, limit=LIMIT, radius=RADIUS)
    assert sorted(got) == sorted(want)
    for key, w in want.items():
        g = got[key]
        assert g.is_cuda, key
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (key, fine_level)
    n_fine, n_nodes = len(host["points"][fine_level]), len(host["points"][-1])
    assert want["table"].shape == (n_nodes, LIMIT) and want["assign"].shape == (n_fine,) and n_nodes > 8
    co = want["corr_offsets"]
    assert len(co) == 3 and co[0] == 0 and co[1] > 0 and co[2] > co[1]                    # both items have overlapping patches
    no = np.concatenate([[0], np.cumsum(host["lengths"][-1])])
    for p in range(2):                                                                    # a pair never leaves its item
        rows = want["node_corr"][co[p]:co[p + 1]]
        assert (rows[:, 0] >= no[2 * p]).all() and (rows[:, 0] < no[2 * p + 1]).all()
        assert (rows[:, 1] >= no[2 * p + 1]).all() and (rows[:, 1] < no[2 * p + 2]).all()
    if fine_level == 0:
        assert (want["sizes"] > LIMIT).any() and (want["table"] == n_fine).any()          # truncated patches and padded ones
    if fine_level == 2:
        assert np.array_equal(want["assign"], np.arange(n_nodes)) and (want["sizes"] == 1).all()
