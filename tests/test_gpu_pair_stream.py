"""`pointreggpt_amd.stream.PairStream` on an MI355X.  Run with `-m gpu`.

The stream must hand out what `Generator.generate(gt_log=True)` writes: the configuration is that of
tests/test_gpu_cloud_finish.py (S = 64, dim 16, 4 DDIM steps of 1000, batches of 2 over 3 scenes, synthetic seed = noise seed
= 11, fp32, keep-probability ~1 with `mask_threshold=0.5`), whose seed is documented to yield gt.log lines on the file path.
The file run is made once per module; everything is compared bit for bit."""
import os

import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

S, DIM, STEPS, BATCH, SCENES = 64, 16, 4, 2, 3
SEED = 11
RADIUS = 0.0375


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


def files_under(root):
    return [os.path.join(d, f) for d, _dirs, fs in os.walk(root) for f in fs]


def make_stream(net, folder, **kw):
    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.stream import PairStream
    diff, mask = net
    gen = Generator(diff, None, batch_size=BATCH, samples_folder=str(folder), synthetic_seed=SEED)
    kw.setdefault("matching_radius", RADIUS)
    return PairStream(gen, mask, start=0, stop=SCENES, noise_seed=SEED, mask_threshold=0.5, **kw)


@pytest.fixture(scope="module")
def on_disk(net, tmp_path_factory):
    """generate(0, 3, 1, gt_log=True) -> per scene (src, tgt, gt.log fields or None)."""
    from pointreggpt_amd.generator import Generator
    diff, mask = net
    data = tmp_path_factory.mktemp("files") / "ds" / "data"
    gen = Generator(diff, None, batch_size=BATCH, samples_folder=str(data), synthetic_seed=SEED)
    gen.generate(0, SCENES, 1, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, gt_log=True)
    out = {}
    for i in range(SCENES):
        sdir = data / "scene-{:0>6d}".format(i)
        lines = (sdir / "gt.log").read_text().splitlines()
        assert len(lines) <= 1
        fields = lines[0].split("\t") if lines else None
        out[i] = (PP.read_ply(str(sdir / "sample-000000.cloud.ply")), PP.read_ply(str(sdir / "sample-000001.cloud.ply")), fields)
    return out


@pytest.fixture(scope="module")
def streamed(net, tmp_path_factory):
    folder = tmp_path_factory.mktemp("stream") / "samples"
    stream = make_stream(net, folder)
    items = list(stream)
    return items, stream, folder


def test_items_are_the_scenes_with_a_gt_log_line(on_disk, streamed):
    items, stream, _ = streamed
    with_line = [i for i in range(SCENES) if on_disk[i][2] is not None]
    assert len(items) >= 1
    assert [it["scene"] for it in items] == with_line
    assert [s for s, _why in stream.skipped] == [i for i in range(SCENES) if on_disk[i][2] is None]
    assert all(isinstance(why, str) and why for _s, why in stream.skipped)


def test_clouds_ratios_and_correspondences(on_disk, streamed):
    items, _, _ = streamed
    for it in items:
        src, tgt, fields = on_disk[it["scene"]]
        assert set(it) == {"scene", "src", "tgt", "overlap_src", "overlap_tgt", "corr"}
        assert isinstance(it["src"], np.ndarray) and it["src"].dtype == np.float64 and it["src"].shape == src.shape
        assert it["tgt"].dtype == np.float64 and it["tgt"].shape == tgt.shape
        assert np.array_equal(bits(it["src"]), bits(src)) and np.array_equal(bits(it["tgt"]), bits(tgt))
        assert isinstance(it["overlap_src"], float) and isinstance(it["overlap_tgt"], float)
        assert fields[:3] == ["scene-{:0>6d}".format(it["scene"]), "0", "1"]
        assert ["{:.4f}".format(it["overlap_src"]), "{:.4f}".format(it["overlap_tgt"])] == fields[3:]
        want = PP.radius_pairs(it["src"], it["tgt"], RADIUS)
        assert len(want) > 0
        assert it["corr"].dtype == np.int32 and np.array_equal(it["corr"], want)
        assert it["src"].flags.owndata and it["tgt"].flags.owndata and it["corr"].flags.owndata


def test_nothing_is_written(streamed):
    _, _, folder = streamed
    assert files_under(str(folder)) == [] and [d for d in os.listdir(str(folder))] == []


def test_without_a_radius_there_is_no_corr(net, streamed, tmp_path):
    items, _, _ = streamed
    got = list(make_stream(net, tmp_path / "s", matching_radius=None))
    assert [g["scene"] for g in got] == [it["scene"] for it in items]
    for g, it in zip(got, items):
        assert "corr" not in g and np.array_equal(bits(g["src"]), bits(it["src"])) and np.array_equal(bits(g["tgt"]), bits(it["tgt"]))


def test_torch_items_hold_the_same_values_on_the_device(net, streamed, tmp_path):
    items, _, _ = streamed
    got = list(make_stream(net, tmp_path / "s", to="torch"))
    assert [g["scene"] for g in got] == [it["scene"] for it in items]
    for g, it in zip(got, items):
        for name, dtype in (("src", torch.float64), ("tgt", torch.float64), ("corr", torch.int32)):
            t = g[name]
            assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
            assert t.untyped_storage().nbytes() == t.numel() * t.element_size()         # owns its memory: no view of a batch buffer
        assert np.array_equal(bits(g["src"].cpu().numpy()), bits(it["src"]))
        assert np.array_equal(bits(g["tgt"].cpu().numpy()), bits(it["tgt"]))
        assert np.array_equal(g["corr"].cpu().numpy(), it["corr"])
        assert (g["overlap_src"], g["overlap_tgt"]) == (it["overlap_src"], it["overlap_tgt"])
    assert files_under(str(tmp_path)) == []


def test_a_second_stream_with_the_same_seeds_yields_the_same_bits(net, streamed, tmp_path):
    items, stream, _ = streamed
    again = make_stream(net, tmp_path / "s")
    got = list(again)
    assert again.skipped == stream.skipped and len(got) == len(items)
    for g, it in zip(got, items):
        assert g["scene"] == it["scene"] and (g["overlap_src"], g["overlap_tgt"]) == (it["overlap_src"], it["overlap_tgt"])
        assert np.array_equal(bits(g["src"]), bits(it["src"])) and np.array_equal(bits(g["tgt"]), bits(it["tgt"]))
        assert np.array_equal(g["corr"], it["corr"])


def test_bad_arguments(net, tmp_path):
    with pytest.raises(ValueError):
        make_stream(net, tmp_path / "s", to="list")
    with pytest.raises(ValueError):
        make_stream(net, tmp_path / "s", matching_radius=0.0)


def test_a_filtered_scene_leaves_the_others_as_they_are(net, streamed, tmp_path, monkeypatch):
    """The pairs that pass the filter are gathered into a buffer of their own for the correspondence search: with one scene of
    the first batch turned away (by a filter patched for this test), every other item keeps its bits."""
    from pointreggpt_amd.generator import Generator
    items, stream, _ = streamed
    victim = items[0]["scene"]
    batch_first = (victim // BATCH) * BATCH
    real = Generator._pair_ratios.__func__

    def picky(cls, offs, d_offs, cnt, j):
        return (None, "turned away by the test") if j == victim - batch_first else real(cls, offs, d_offs, cnt, j)

    monkeypatch.setattr(Generator, "_pair_ratios", classmethod(picky))
    again = make_stream(net, tmp_path / "s")
    got = list(again)
    dropped = {s for s, why in again.skipped if why == "turned away by the test"}
    assert victim in dropped
    want = [it for it in items if it["scene"] not in dropped]
    assert [g["scene"] for g in got] == [it["scene"] for it in want]
    for g, it in zip(got, want):
        assert np.array_equal(bits(g["src"]), bits(it["src"])) and np.array_equal(bits(g["tgt"]), bits(it["tgt"]))
        assert np.array_equal(g["corr"], it["corr"])
