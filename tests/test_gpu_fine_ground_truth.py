"""geometry.fine_ground_truth and geometry.select_node_corr on an MI355X against their specifications in postprocess, bit for bit.
Run with `-m gpu`.  The label kernel has its own test (tests/test_gpu_fine_labels.py); what is checked here is the layer on the
pyramid and on the coarse ground truth: the selection by keys, the gathers, the masks, and the generator path."""
import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

KW = dict(num_stages=3, voxel_size=0.025, radius=0.0625, neighbor_limits=(20, 20, 20))
LIMIT, RADIUS = 8, 0.05
SELECT = dict(min_overlap=0.3, num_targets=64)


def voxel_like(rng, n):
    """tests/test_gpu_coarse_ground_truth.py's clouds: a 2.5 cm grid surface patch and the same patch with a 1 cm jitter."""
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 0.025
    a = np.concatenate([g, 1.5 + 0.1 * np.sin(3 * g[:, :1])], 1) + rng.uniform(-0.004, 0.004, (n, 3))
    b = a + rng.normal(0, 0.01, (n, 3))
    return a, b[rng.permutation(n)][: n - n // 10]


@pytest.fixture(scope="module")
def world():
    """Two items of ~600-row clouds in float32: the host pyramid and per fine level its coarse ground truth (the reference,
    computed once), and the same two on the device."""
    from pointreggpt_amd import geometry as G
    rng = np.random.default_rng(31)
    clouds = [c for n in (620, 577) for c in voxel_like(rng, n)]
    pts32 = np.concatenate(clouds).astype(np.float32)
    lens = [len(c) for c in clouds]
    host = PP.neighbor_pyramid(pts32, lens, KW["num_stages"], KW["voxel_size"], KW["radius"], KW["neighbor_limits"])
    dev = G.neighbor_pyramid(torch.from_numpy(pts32).cuda(), lens, **KW)
    host_gt = [PP.coarse_ground_truth(host, fine_level=l, limit=LIMIT, radius=RADIUS) for l in range(3)]
    dev_gt = [G.coarse_ground_truth(dev, fine_level=l, limit=LIMIT, radius=RADIUS) for l in range(3)]
    return host, dev, host_gt, dev_gt


def same(got, want, what):
    assert got.is_cuda, what
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape and g.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("fine_level", [0, 1, 2])
def test_fine_ground_truth_equals_the_specification(world, fine_level):
    from pointreggpt_amd import geometry as G
    host, dev, host_gt, dev_gt = world
    keys = np.random.default_rng(100 + fine_level).random(len(host_gt[fine_level]["overlap"]))
    want = PP.fine_ground_truth(host, host_gt[fine_level], fine_level=fine_level, radius=RADIUS, keys=keys, **SELECT)
    got = G.fine_ground_truth(dev, dev_gt[fine_level], fine_level=fine_level, radius=RADIUS, keys=torch.from_numpy(keys).cuda(),
                              **SELECT)
    assert sorted(got) == sorted(want)
    for key, w in want.items():
        same(got[key], w, (key, fine_level))
    counts = np.diff(want["sel_offsets"]).tolist()
    assert counts == ([53, 43] if fine_level == 2 else [64, 64])                          # all kept / truncated by the keys
    assert want["labels"][:, :LIMIT, :LIMIT].any(axis=(1, 2)).all()                       # a listed pair has a match
    if fine_level == 0:
        assert want["labels"][:, :LIMIT, LIMIT].any() and (~want["src_mask"]).any()       # slack rows and padded patches


def test_select_node_corr_alone(world):
    from pointreggpt_amd import geometry as G
    _, _, host_gt, dev_gt = world
    gt, d_gt = host_gt[0], dev_gt[0]
    P = len(gt["overlap"])
    rng = np.random.default_rng(5)
    for keys, kw in ((rng.random(P), dict(min_overlap=0.1, num_targets=128)),             # the defaults
                     (rng.random(P), dict(min_overlap=0.3, num_targets=64)),
                     (rng.integers(0, 4, P).astype(np.float64), dict(min_overlap=0.2, num_targets=7)),     # ties go by row
                     (np.zeros(P), dict(min_overlap=0.0, num_targets=1)),
                     (rng.random(P), dict(min_overlap=2.0, num_targets=5))):              # no candidate anywhere
        w_rows, w_so = PP.select_node_corr(gt["overlap"], gt["corr_offsets"], keys, **kw)
        rows, so = G.select_node_corr(d_gt, keys=torch.from_numpy(keys).cuda(), **kw)
        same(rows, w_rows, kw)
        same(so, w_so, kw)
    # an item without rows and one without candidates, on a hand-made ground truth
    ov = np.array([0.5, 0.1, 0.30000001, 0.05, 0.9, 0.1, 0.02, 0.4, 0.4, 0.4, 0.4, 0.11, 0.7, 0.1])
    co = np.array([0, 5, 7, 7, 14], dtype=np.int64)
    ky = np.array([0.9, 0.0, 0.1, 0.0, 0.5, 0.0, 0.0, 0.25, 0.75, 0.25, 0.25, 0.8, 0.1, 0.0])
    small = {"overlap": torch.from_numpy(ov).cuda(), "corr_offsets": torch.from_numpy(co).cuda()}
    for k in (1, 3, 4, 100):
        w_rows, w_so = PP.select_node_corr(ov, co, ky, min_overlap=0.1, num_targets=k)
        rows, so = G.select_node_corr(small, min_overlap=0.1, num_targets=k, keys=torch.from_numpy(ky).cuda())
        same(rows, w_rows, k)
        same(so, w_so, k)
    assert PP.select_node_corr(ov, co, ky, min_overlap=0.1, num_targets=3)[0].tolist() == [0, 2, 4, 7, 9, 12]


def test_generator_path_is_reproducible_and_samples_the_candidates(world):
    from pointreggpt_amd import geometry as G
    host, dev, host_gt, dev_gt = world
    gt, d_gt = host_gt[0], dev_gt[0]
    co = gt["corr_offsets"]
    outs = []
    for seed in (11, 11, 12):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        outs.append(G.fine_ground_truth(dev, d_gt, fine_level=0, radius=RADIUS, generator=gen, **SELECT))
    for key in outs[0]:
        assert torch.equal(outs[0][key], outs[1][key]), key                               # the same seed, the same result
    assert not torch.equal(outs[0]["rows"], outs[2]["rows"])                              # 64 of ~140 per item: another sample
    rows, so = outs[0]["rows"].cpu().numpy(), outs[0]["sel_offsets"].cpu().numpy()
    cand = gt["overlap"] > SELECT["min_overlap"]
    assert cand[rows].all() and (np.diff(rows) > 0).all()
    for p in range(2):
        mine = rows[so[p]:so[p + 1]]
        assert ((mine >= co[p]) & (mine < co[p + 1])).all()
        assert len(mine) == min(int(cand[co[p]:co[p + 1]].sum()), SELECT["num_targets"]) == 64
    # the labels of a sampled selection are the specification's for those rows
    want = PP.patch_corr_labels(np.asarray(host["points"][0], dtype=np.float64), gt["table"], gt["node_corr"][rows], RADIUS)
    assert np.array_equal(outs[0]["labels"].cpu().numpy(), want)
