"""`PairStream(augment=Augment(...), epoch=...)` on an MI355X.  Run with `-m gpu`.

The configuration is that of tests/test_gpu_pair_stream.py (S = 64, dim 16, 4 DDIM steps of 1000, 3 scenes, synthetic seed =
noise seed = 11, fp32, `mask_threshold=0.5`).  The plain stream is run once per module; an augmented item must be, bit for bit,
`postprocess.augment_cloud` of the plain item's clouds with the documented seeds (`synthetic.augment_seed`) and poses
(`stream.augment_poses`), and its `corr` the numpy search on those clouds under `transform`."""
import numpy as np
import pytest

from pointreggpt_amd import postprocess as PP
from pointreggpt_amd import synthetic

pytestmark = pytest.mark.gpu

S, DIM, STEPS, SCENES = 64, 16, 4, 3
SEED = 11
RADIUS = 0.0375
NOISE = 0.005
LIMIT = 1000            # below the smallest finished cloud of these scenes (asserted), so every cloud is cut


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def net():
    from pointreggpt_amd import _lib
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.unet import MaskUnet, Unet
    _lib.load()
    unet = Unet(DIM, dtype="fp32").init_synthetic(3)
    mask = MaskUnet(DIM, dtype="fp32").init_synthetic(4, final_bias=8.0)
    diff = GaussianDiffusion(unet, image_size=S, timesteps=1000, sampling_timesteps=STEPS)
    yield diff, mask
    diff.close(); unet.close(); mask.close()


def run_stream(net, folder, batch_size=2, **kw):
    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.stream import PairStream
    diff, mask = net
    gen = Generator(diff, None, batch_size=batch_size, samples_folder=str(folder), synthetic_seed=SEED)
    return list(PairStream(gen, mask, start=0, stop=SCENES, noise_seed=SEED, mask_threshold=0.5, matching_radius=RADIUS, **kw))


def augment():
    from pointreggpt_amd.stream import Augment
    return Augment(noise=NOISE, point_limit=LIMIT, rotation="both")


@pytest.fixture(scope="module")
def plain(net, tmp_path_factory):
    items = run_stream(net, tmp_path_factory.mktemp("plain") / "s")
    assert len(items) >= 1
    return items


@pytest.fixture(scope="module")
def augmented(net, tmp_path_factory):
    return run_stream(net, tmp_path_factory.mktemp("aug") / "s", augment=augment())


def same_items(a, b):
    assert [x["scene"] for x in a] == [y["scene"] for y in b]
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            if k in ("src", "tgt", "transform"):
                assert np.array_equal(bits(x[k]), bits(y[k])), k
            elif k in ("corr", "src_rows", "tgt_rows"):
                assert x[k].dtype == np.int32 and np.array_equal(x[k], y[k]), k
            else:
                assert x[k] == y[k], k


def test_items_are_the_specification_of_the_plain_items(plain, augmented):
    from pointreggpt_amd.stream import augment_poses
    smallest = min(min(len(it["src"]), len(it["tgt"])) for it in plain)
    print("finished cloud sizes:", [(len(it["src"]), len(it["tgt"])) for it in plain])
    assert LIMIT < smallest
    assert [a["scene"] for a in augmented] == [p["scene"] for p in plain]
    for a, p in zip(augmented, plain):
        assert set(a) == set(p) | {"transform", "src_rows", "tgt_rows"}
        move_src, move_tgt, transform = augment_poses(SEED, p["scene"], 0, augment())
        src, src_rows = PP.augment_cloud(p["src"], seed=synthetic.augment_seed(SEED, p["scene"], 0), draw=0, noise=NOISE,
                                         limit=LIMIT, T=move_src)
        tgt, tgt_rows = PP.augment_cloud(p["tgt"], seed=synthetic.augment_seed(SEED, p["scene"], 1), draw=0, noise=NOISE,
                                         limit=LIMIT, T=move_tgt)
        assert a["src"].shape == (LIMIT, 3) and a["tgt"].shape == (LIMIT, 3)
        assert a["src_rows"].dtype == np.int32 and np.array_equal(a["src_rows"], src_rows)
        assert a["tgt_rows"].dtype == np.int32 and np.array_equal(a["tgt_rows"], tgt_rows)
        assert np.array_equal(bits(a["src"]), bits(src)) and np.array_equal(bits(a["tgt"]), bits(tgt))
        assert a["transform"].dtype == np.float64 and np.array_equal(bits(a["transform"]), bits(transform))
        want = PP.radius_pairs(PP.rigid_move(src, transform), tgt, RADIUS)
        assert a["corr"].dtype == np.int32 and np.array_equal(a["corr"], want)
        assert (a["overlap_src"], a["overlap_tgt"]) == (p["overlap_src"], p["overlap_tgt"])
        for k in ("src", "tgt", "corr", "src_rows", "tgt_rows"):
            assert a[k].flags.owndata, k
        # the moved source lies on the target again: the noise and nothing else separates it from the un-augmented geometry
        back = PP.rigid_move(a["src"], a["transform"])
        assert np.abs(back - PP.rigid_move(p["src"][src_rows], move_tgt)).max() < NOISE
    assert sum(len(a["corr"]) for a in augmented) > 0


def test_batch_size_does_not_change_an_item(net, augmented, tmp_path):
    same_items(run_stream(net, tmp_path / "s", batch_size=1, augment=augment()), augmented)


def test_another_epoch_is_another_augmentation(net, augmented, tmp_path):
    other = run_stream(net, tmp_path / "s", augment=augment(), epoch=1)
    assert [o["scene"] for o in other] == [a["scene"] for a in augmented]
    for o, a in zip(other, augmented):
        assert not np.array_equal(o["src_rows"], a["src_rows"]) and not np.array_equal(o["tgt_rows"], a["tgt_rows"])
        assert not np.array_equal(bits(o["transform"]), bits(a["transform"]))
        assert not np.array_equal(bits(o["src"]), bits(a["src"])) and not np.array_equal(bits(o["tgt"]), bits(a["tgt"]))


def test_without_augment_the_items_are_todays(net, plain, tmp_path):
    got = run_stream(net, tmp_path / "s", augment=None, epoch=5)
    assert all(set(g) == {"scene", "src", "tgt", "overlap_src", "overlap_tgt", "corr"} for g in got)
    same_items(got, plain)


def test_torch_items_hold_the_same_values_on_the_device(net, augmented, tmp_path):
    import torch
    got = run_stream(net, tmp_path / "s", augment=augment(), to="torch")
    assert [g["scene"] for g in got] == [a["scene"] for a in augmented]
    for g, a in zip(got, augmented):
        for k, dtype in (("src", torch.float64), ("tgt", torch.float64), ("transform", torch.float64), ("corr", torch.int32),
                         ("src_rows", torch.int32), ("tgt_rows", torch.int32)):
            t = g[k]
            assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
            assert t.untyped_storage().nbytes() == t.numel() * t.element_size()     # owns its memory: no view of a batch buffer
            assert np.array_equal(t.cpu().numpy(), a[k]), k
