"""Per-view clouds on an MI355X: prg_overlap_counts_indexed alone, `Generator.generate(clouds="per_view")` on every route, and
`PairStream(num_samples=k, clouds="per_view")`.  Run with `-m gpu`.

Everything is compared bit for bit / byte for byte; no tolerance is involved.  The configuration is that of
tests/test_gpu_cloud_finish.py and tests/test_gpu_pair_stream.py: S = 64, dim 16, 4 DDIM steps of 1000, batches of 2 over 3
scenes, fp32 synthetic weights, `mask_threshold=0.5`, synthetic seed = noise seed = SEED = 11.  With seed 11 the `device="cpu"`
generator followed by `generate_gt(num_samples=3, overlap="numpy-spec")` lists all three pairs (0, 1), (0, 2) and (1, 2) of
every scene (tests/test_per_view_host.py runs that path), so 11 is kept; the assertion that the logs hold lines with s = 0 and
lines with s >= 1 is made here on the device's own files either way.  Every dataset is generated once per module."""
import os
from itertools import combinations

import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP
from pointreggpt_amd import synthetic

pytestmark = pytest.mark.gpu

S, DIM, STEPS, BATCH, SCENES = 64, 16, 4, 2, 3
SEED = 11
RADIUS = 0.0375
NOISE = 0.005
LIMIT = 900             # below generate_gt's 1000-row floor: every cloud of a listed pair is cut


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------
SIZES = [0, 1, 255, 256, 257, 700]                  # 255 / 256 / 257: the edges of a 256-query slab and a 256-row tile
HEAD, TAIL = 5, 9
PAIRS = [(5, 2), (2, 5), (5, 3), (3, 3), (5, 4), (2, 6), (4, 5), (1, 5), (0, 5), (2, 3), (4, 4)]       # (2, 6): cloud 6 does not exist
BAD = 5


def kernel_case():
    rng = np.random.RandomState(2024)
    clouds = [rng.uniform(0.0, 1.0, (n, 3)) for n in SIZES]
    clouds[1][0] = clouds[5][17] + 0.01               # the single row has neighbours at any radius of interest
    clouds[3][7] = np.nan                             # one NaN row: it has no neighbour and is nobody's
    offs = np.zeros(len(SIZES) + 1, dtype=np.int64)
    offs[0] = HEAD
    offs[1:] = HEAD + np.cumsum(SIZES)
    poison = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]
    pts = np.concatenate([np.full((HEAD, 3), poison)] + clouds + [np.full((TAIL, 3), poison)], 0)
    return clouds, pts, offs


def numpy_counts(a, b, r):
    """(rows of a with a row of b strictly within r, the same from b's side): dx*dx + dy*dy + dz*dz < r*r."""
    if len(a) == 0 or len(b) == 0:
        return 0, 0
    with np.errstate(invalid="ignore"):
        dx, dy, dz = b[None, :, 0] - a[:, None, 0], b[None, :, 1] - a[:, None, 1], b[None, :, 2] - a[:, None, 2]
        hit = dx * dx + dy * dy + dz * dz < r * r
    return int(hit.any(axis=1).sum()), int(hit.any(axis=0).sum())


def test_indexed_counts_against_numpy_and_the_adjacent_kernel():
    from pointreggpt_amd import _lib
    from pointreggpt_amd import geometry as G
    lib = _lib.load()
    clouds, pts, offs = kernel_case()
    good = [p for k, p in enumerate(PAIRS) if k != BAD]
    assert sum(5 in p for p in good) >= 4 and (5, 2) in good and (2, 5) in good and (3, 3) in good and 0 < BAD < len(PAIRS) - 1

    def mixed(r):           # pairs whose two counts are both neither 0 nor the whole cloud
        return sum(0 < c[0] < len(clouds[s]) and 0 < c[1] < len(clouds[t])
                   for (s, t) in good for c in [numpy_counts(clouds[s], clouds[t], r)])

    radius = next(r for r in (0.08, 0.06, 0.1, 0.04) if 2 * mixed(r) >= len(PAIRS))       # chosen on the CPU, from numpy's counts
    assert 2 * mixed(radius) >= len(PAIRS)
    want = np.array([(-1, -1) if k == BAD else numpy_counts(clouds[s], clouds[t], radius) for k, (s, t) in enumerate(PAIRS)])
    d_pts, d_offs = D(pts), D(offs)
    got = G.overlap_counts_indexed(d_pts, d_offs, D(np.array(PAIRS, dtype=np.int32)), max(SIZES), radius)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    print("radius", radius, "counts", got.tolist())
    assert got.dtype == np.int32 and got.shape == (len(PAIRS), 2)
    assert np.array_equal(got, want)
    assert tuple(got[BAD]) == (-1, -1) and np.array_equal(got[BAD - 1], want[BAD - 1]) and np.array_equal(got[BAD + 1], want[BAD + 1])
    assert tuple(got[PAIRS.index((3, 3))]) == (255, 255) and tuple(got[PAIRS.index((4, 4))]) == (257, 257)   # s == t: finite rows once
    assert tuple(got[PAIRS.index((2, 5))]) == tuple(got[PAIRS.index((5, 2))])[::-1]
    assert np.array_equal(bits(d_pts.cpu().numpy()), bits(pts))                         # nothing but the counts is written
    # prg_overlap_counts on the same pairs, every cloud copied once per pair into the adjacent layout
    flat = [clouds[c] for p in good for c in p]
    a_offs = np.concatenate([[0], np.cumsum([len(c) for c in flat])]).astype(np.int64)
    adjacent = torch.empty((len(good), 2), dtype=torch.int32, device="cuda")
    a_pts, a_offs = D(np.concatenate(flat, 0)), D(a_offs)               # named: both must be alive when the call is made
    _lib.check(lib.prg_overlap_counts(_lib.ptr(a_pts), _lib.ptr(a_offs), len(good), max(SIZES), radius, _lib.ptr(adjacent),
                                      _lib.stream_ptr()), "prg_overlap_counts")
    torch.cuda.synchronize()
    assert np.array_equal(adjacent.cpu().numpy(), np.delete(got, BAD, axis=0))
    # a negative entry is outside too, in either position, and a list may be nothing but such pairs
    got = G.overlap_counts_indexed(d_pts, d_offs, D(np.array([(-1, 2), (5, 2), (2, -2 ** 31)], dtype=np.int32)), max(SIZES), radius)
    assert got.cpu().numpy().tolist() == [[-1, -1], list(want[0]), [-1, -1]]


def test_overlap_ratios_indexed_are_the_ratios_of_every_pair():
    rng = np.random.RandomState(7)
    clouds = [rng.uniform(0.0, 0.6, (n, 3)) for n in (1500, 0, 2100, 900)]
    pairs = [(0, 2), (0, 3), (2, 3), (3, 2), (1, 0), (2, 2)]
    flat = [(clouds[s], clouds[t]) for s, t in pairs]
    want = PP.overlap_ratios_hip(flat)                                  # every cloud uploaded and gridded once per pair
    for (s, t), w in zip(pairs, want):
        if 1 not in (s, t):                                             # (the numpy specification takes no empty cloud)
            assert w == PP.compute_overlap_ratio(clouds[s], clouds[t]), (s, t)
    for voxel in ("device", "host"):
        got = PP.overlap_ratios_indexed_hip(clouds, pairs, voxel=voxel)
        assert len(got) == len(pairs)
        for g, w in zip(got, want):
            assert np.array_equal(np.array(g).view(np.uint64), np.array(w).view(np.uint64)), (voxel, g, w)
    assert 0 < want[0][0] < 1 and np.isnan(want[4][0]) and want[5] == (1.0, 1.0)
    with pytest.raises(ValueError):
        PP.overlap_ratios_indexed_hip(clouds, [(0, 4)])
    assert PP.overlap_ratios_indexed_hip(clouds, []) == []


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def tree(root):
    out = {}
    for d, _dirs, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def nets():
    """Two sets of the same networks on their own handles: the second is a lane."""
    from pointreggpt_amd import _lib
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.unet import MaskUnet, Unet
    _lib.load()
    made = []
    for _ in range(2):
        unet = Unet(DIM, dtype="fp32").init_synthetic(3)
        mask = MaskUnet(DIM, dtype="fp32").init_synthetic(4, final_bias=8.0)
        made.append((GaussianDiffusion(unet, image_size=S, timesteps=1000, sampling_timesteps=STEPS), unet, mask))
    yield [(diff, mask) for diff, _unet, mask in made]
    for diff, unet, mask in made:
        diff.close(); unet.close(); mask.close()


@pytest.fixture(scope="module")
def net(nets):
    return nets[0]


@pytest.fixture(scope="module")
def dataset(net, tmp_path_factory):
    """dataset(k, clouds, gt_log, voxel_backend) -> the root of that run's dataset `ds`, generated once."""
    from pointreggpt_amd.generator import Generator
    diff, mask = net
    made = {}

    def get(k, clouds, gt_log, voxel_backend="device"):
        key = (k, clouds, gt_log, voxel_backend)
        if key not in made:
            root = tmp_path_factory.mktemp("k{}_{}_{}_{}".format(k, clouds, "gt" if gt_log else "plain", voxel_backend))
            gen = Generator(diff, None, batch_size=BATCH, samples_folder=str(root / "ds" / "data"), synthetic_seed=SEED)
            gen.generate(0, SCENES, k, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, gt_log=gt_log, clouds=clouds,
                         voxel_backend=voxel_backend)
            made[key] = root
        return made[key]

    return get


@pytest.mark.parametrize("gt_log", [True, False])
def test_one_view_per_scene_is_the_fused_dataset(dataset, gt_log):
    a, b = tree(str(dataset(1, "fused", gt_log))), tree(str(dataset(1, "per_view", gt_log)))
    assert sorted(a) == sorted(b) and len(a) == SCENES * (10 if gt_log else 9)
    for name in a:
        assert a[name] == b[name], name


def gt_logs(root, overlap):
    """The scene logs `generate_gt(num_samples=3, overlap=)` writes for the dataset under `root`, which is left as it was."""
    from pointreggpt_amd.generator import generate_gt
    generate_gt("ds", 0, SCENES, 3, root=str(root), overlap=overlap)
    logs = {}
    for i in range(SCENES):
        p = root / "ds" / "data" / "scene-{:0>6d}".format(i) / "gt.log"
        logs[i] = p.read_bytes()
        os.remove(str(p))
    return logs


@pytest.fixture(scope="module")
def one_pass(dataset):
    root = dataset(2, "per_view", True)
    return root, tree(str(root))


@pytest.mark.parametrize("voxel_backend", ["device", "host"])
def test_two_views_one_pass_leaves_the_files_of_two(dataset, one_pass, voxel_backend):
    _, b = one_pass
    root = dataset(2, "per_view", False, voxel_backend)
    a = tree(str(root))
    logs = {"ds/data/scene-{:0>6d}/gt.log".format(i) for i in range(SCENES)}
    assert set(b) - set(a) == logs and set(a) <= set(b) and len(a) == SCENES * 13
    assert sum(n.endswith(".cloud.ply") for n in a) == 3 * SCENES
    for name in a:
        assert a[name] == b[name], name
    for overlap in ("hip", "numpy-spec"):
        two = gt_logs(root, overlap)
        for i in range(SCENES):
            assert two[i] == b["ds/data/scene-{:0>6d}/gt.log".format(i)], (overlap, i)


def log_lines(files):
    return [ln.split("\t") for i in range(SCENES) for ln in files["ds/data/scene-{:0>6d}/gt.log".format(i)].decode().splitlines()]


def test_the_logs_hold_pairs_with_the_source_frame_and_pairs_of_two_views(one_pass):
    _, b = one_pass
    lines = log_lines(b)
    print("gt.log lines:", ["\t".join(ln) for ln in lines])
    order = list(combinations(range(3), 2))
    for i in range(SCENES):
        got = [(int(s), int(t)) for n, s, t, _o1, _o2 in lines if n == "scene-{:0>6d}".format(i)]
        assert got == [p for p in order if p in got]                                       # `combinations` order, no repeats
    assert any(int(s) == 0 for _n, s, _t, _o1, _o2 in lines)
    assert any(int(s) >= 1 for _n, s, _t, _o1, _o2 in lines)                               # a pair of two generated views
    for _n, _s, _t, o1, o2 in lines:
        assert len(o1.split(".")[1]) == 4 and len(o2.split(".")[1]) == 4


@pytest.mark.parametrize("gt_log", [True, False])
def test_two_lanes_leave_the_same_per_view_files(dataset, nets, gt_log, tmp_path):
    from pointreggpt_amd.generator import Generator
    (diff, mask), lane = nets
    gen = Generator(diff, None, batch_size=BATCH, samples_folder=str(tmp_path / "ds" / "data"), synthetic_seed=SEED)
    stats = {}
    gen.generate(0, SCENES, 2, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, gt_log=gt_log, clouds="per_view",
                 lanes=[lane], stats=stats)
    assert stats["lanes"] == 2
    assert tree(str(tmp_path)) == tree(str(dataset(2, "per_view", gt_log)))


def test_the_fused_mode_with_two_views_is_what_it_was(dataset, one_pass):
    """`clouds="fused"` with two views: two clouds and the pair (0, 1); everything but the target cloud and the log is shared."""
    _, b = one_pass
    fused = tree(str(dataset(2, "fused", True)))
    assert not any(n.endswith("sample-000002.cloud.ply") for n in fused)
    assert all((s, t) == ("0", "1") for _n, s, t, _o1, _o2 in log_lines(fused))
    for name in fused:
        if not name.endswith("sample-000001.cloud.ply") and not name.endswith("gt.log"):
            assert fused[name] == b[name], name


# ---- 5. the stream ---------------------------------------------------------------------------------------------------------------
def run_stream(net, folder, batch_size=BATCH, **kw):
    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.stream import PairStream
    diff, mask = net
    gen = Generator(diff, None, batch_size=batch_size, samples_folder=str(folder), synthetic_seed=SEED)
    kw.setdefault("num_samples", 2)
    kw.setdefault("clouds", "per_view")
    stream = PairStream(gen, mask, start=0, stop=SCENES, noise_seed=SEED, mask_threshold=0.5, matching_radius=RADIUS, **kw)
    return list(stream), stream


@pytest.fixture(scope="module")
def streamed(net, tmp_path_factory):
    return run_stream(net, tmp_path_factory.mktemp("stream") / "s")


def test_stream_items_are_the_files_of_the_one_pass_run(one_pass, streamed):
    root, b = one_pass
    items, stream = streamed
    lines = log_lines(b)
    assert len(items) == len(lines) >= 2
    assert [(it["scene"], it["src_idx"], it["tgt_idx"]) for it in items] == [(int(n[-6:]), int(s), int(t)) for n, s, t, _o1, _o2 in lines]
    for it, (name, s, t, o1, o2) in zip(items, lines):
        assert set(it) == {"scene", "src", "tgt", "overlap_src", "overlap_tgt", "corr", "src_idx", "tgt_idx"}
        src, tgt = (PP.read_ply(str(root / "ds" / "data" / name / "sample-{:0>6d}.cloud.ply".format(int(k)))) for k in (s, t))
        assert it["src"].dtype == np.float64 and it["src"].shape == src.shape and it["tgt"].shape == tgt.shape
        assert np.array_equal(bits(it["src"]), bits(src)) and np.array_equal(bits(it["tgt"]), bits(tgt))
        assert isinstance(it["overlap_src"], float) and ["{:.4f}".format(it["overlap_src"]), "{:.4f}".format(it["overlap_tgt"])] == [o1, o2]
        want = PP.radius_pairs(it["src"], it["tgt"], RADIUS)
        assert len(want) > 0 and it["corr"].dtype == np.int32 and np.array_equal(it["corr"], want)
        assert it["src"].flags.owndata and it["tgt"].flags.owndata and it["corr"].flags.owndata
    listed = {(int(n[-6:]), int(s), int(t)) for n, s, t, _o1, _o2 in lines}
    dropped = [(i, s, t) for i in range(SCENES) for s, t in combinations(range(3), 2) if (i, s, t) not in listed]
    assert [scene for scene, _why in stream.skipped] == [i for i, _s, _t in dropped]
    for (scene, why), (_i, s, t) in zip(stream.skipped, dropped):
        assert why.startswith("pair ({}, {}): ".format(s, t)) and len(why) > len("pair (0, 1): ")


def test_a_second_stream_and_another_batch_size_yield_the_same_bits(net, streamed, tmp_path):
    items, stream = streamed
    for batch_size in (BATCH, 1):
        got, again = run_stream(net, tmp_path / "s{}".format(batch_size), batch_size=batch_size)
        assert again.skipped == stream.skipped and len(got) == len(items)
        for g, it in zip(got, items):
            assert (g["scene"], g["src_idx"], g["tgt_idx"], g["overlap_src"], g["overlap_tgt"]) == \
                   (it["scene"], it["src_idx"], it["tgt_idx"], it["overlap_src"], it["overlap_tgt"])
            assert np.array_equal(bits(g["src"]), bits(it["src"])) and np.array_equal(bits(g["tgt"]), bits(it["tgt"]))
            assert np.array_equal(g["corr"], it["corr"])
    assert os.listdir(str(tmp_path / "s1")) == []                                           # nothing is written


def test_a_fused_stream_of_two_views_is_the_fused_one_pass_run(dataset, net, tmp_path):
    root = dataset(2, "fused", True)
    lines = log_lines(tree(str(root)))
    items, _ = run_stream(net, tmp_path / "s", clouds="fused")
    assert [it["scene"] for it in items] == [int(n[-6:]) for n, _s, _t, _o1, _o2 in lines] and len(items) >= 1
    for it, (name, _s, _t, o1, o2) in zip(items, lines):
        assert set(it) == {"scene", "src", "tgt", "overlap_src", "overlap_tgt", "corr"}
        src, tgt = (PP.read_ply(str(root / "ds" / "data" / name / "sample-{:0>6d}.cloud.ply".format(k))) for k in (0, 1))
        assert np.array_equal(bits(it["src"]), bits(src)) and np.array_equal(bits(it["tgt"]), bits(tgt))
        assert ["{:.4f}".format(it["overlap_src"]), "{:.4f}".format(it["overlap_tgt"])] == [o1, o2]


# ---- 6. the augmented stream -----------------------------------------------------------------------------------------------------
def test_augmented_items_are_the_specification_with_the_keys_of_their_pair(net, streamed, tmp_path):
    from pointreggpt_amd.stream import Augment, augment_poses
    plain, _ = streamed
    aug = Augment(noise=NOISE, point_limit=LIMIT, rotation="both")
    items, _ = run_stream(net, tmp_path / "s", augment=aug, epoch=3)
    assert [(a["scene"], a["src_idx"], a["tgt_idx"]) for a in items] == [(p["scene"], p["src_idx"], p["tgt_idx"]) for p in plain]
    for a, p in zip(items, plain):
        pair = (p["src_idx"], p["tgt_idx"])
        assert set(a) == set(p) | {"transform", "src_rows", "tgt_rows"}
        move_src, move_tgt, transform = augment_poses(SEED, p["scene"], 3, aug, pair=pair)
        src, src_rows = PP.augment_cloud(p["src"], seed=synthetic.augment_seed_pair(SEED, p["scene"], 0, pair=pair), draw=3, noise=NOISE,
                                         limit=LIMIT, T=move_src)
        tgt, tgt_rows = PP.augment_cloud(p["tgt"], seed=synthetic.augment_seed_pair(SEED, p["scene"], 1, pair=pair), draw=3, noise=NOISE,
                                         limit=LIMIT, T=move_tgt)
        assert a["src"].shape == (LIMIT, 3) and a["tgt"].shape == (LIMIT, 3)
        assert np.array_equal(a["src_rows"], src_rows) and np.array_equal(a["tgt_rows"], tgt_rows)
        assert np.array_equal(bits(a["src"]), bits(src)) and np.array_equal(bits(a["tgt"]), bits(tgt))
        assert np.array_equal(bits(a["transform"]), bits(transform))
        assert np.array_equal(a["corr"], PP.radius_pairs(PP.rigid_move(src, transform), tgt, RADIUS))   # corr holds under `transform`
        assert (a["overlap_src"], a["overlap_tgt"]) == (p["overlap_src"], p["overlap_tgt"])
    assert sum(len(a["corr"]) for a in items) > 0
    by_scene = {}
    for a in items:
        by_scene.setdefault(a["scene"], []).append(a)
    several = [v for v in by_scene.values() if len(v) >= 2]
    assert several                                                                          # two pairs of one scene:
    for v in several:
        for x, y in combinations(v, 2):
            assert not np.array_equal(bits(x["transform"]), bits(y["transform"]))           # independent draws
