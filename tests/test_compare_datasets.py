"""pointreggpt_amd.compare / compare_datasets.py: two dataset trees compared cloud by cloud and gt.log line by line.

The CPU tests write two tiny trees themselves (write_ply + hand-written gt.log files) and run `backend="numpy-spec"`; the
GPU tests (marked) ask the HIP backend for the same report, float for float, and compare trees that `Generator.generate`
wrote.  All coordinates and the shift below are multiples of 1/64, so every distance is exact in float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pointreggpt_amd import postprocess as PP
from pointreggpt_amd.compare import compare_datasets, read_gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT = np.array([1.0, 2.0, -2.0]) / 64            # length 3/64 = 0.046875 exactly; the grids below have a spacing of 1/8
SHIFT_LEN = 3.0 / 64
SCENES = 3


def grid(nx, ny, nz, origin):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g / 8.0 + np.asarray(origin, dtype=np.float64)


def scene_clouds(scene):
    """Two clouds per scene whose sizes differ per scene and sample (126 .. 330 rows)."""
    return [grid(6 + scene, 7, 3, (-1.0, -0.5, 1.0 + scene)), grid(5, 6 + scene, 11 - scene, (0.25, -1.0, 0.5))]


def write_tree(root, shift=None, skip=(), gt=None, gathered=False):
    """`gt`: {scene: [(s, t, overlap_src, overlap_tgt), ...]} -> the scenes' gt.log files, or metadata/gt.log if `gathered`."""
    for scene in range(SCENES):
        sdir = root / "data" / "scene-{:0>6d}".format(scene)
        sdir.mkdir(parents=True)
        for k, pts in enumerate(scene_clouds(scene)):
            if (scene, k) not in skip:
                PP.write_ply(str(sdir / "sample-{:0>6d}.cloud.ply".format(k)), pts if shift is None else pts + shift)
    lines = {s: ["scene-{:0>6d}\t{}\t{}\t{:.4f}\t{:.4f}\n".format(s, *ln) for ln in lns] for s, lns in (gt or {}).items()}
    if gathered:
        (root / "metadata").mkdir()
        (root / "metadata" / "gt.log").write_text("".join("".join(lines[s]) for s in sorted(lines)))
    else:
        for s, lns in lines.items():
            (root / "data" / "scene-{:0>6d}".format(s) / "gt.log").write_text("".join(lns))
    return root


GT_A = {0: [(0, 1, 0.5, 0.625)], 1: [(0, 1, 0.75, 0.875)]}
GT_B = {0: [(0, 1, 0.4375, 0.6875)], 2: [(0, 1, 0.25, 0.125)]}


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp("trees")
    return {"a": write_tree(base / "a", gt=GT_A, gathered=True), "same": write_tree(base / "same", gt=GT_A),
            "shifted": write_tree(base / "shifted", shift=SHIFT, gt=GT_B),
            "holes": write_tree(base / "holes", skip={(1, 1)}, gt=GT_A), "base": base}


def test_identical_trees(trees):
    rep = compare_datasets(trees["a"], trees["same"], 0, SCENES, backend="numpy-spec")
    s = rep["summary"]
    assert s["identical"] is True and s["compared"] == 2 * SCENES and s["missing_a"] == s["missing_b"] == s["empty"] == 0
    for name in ("chamfer", "hausdorff", "p50", "p95", "p99"):
        assert s[name] == {"median": 0.0, "p95": 0.0, "max": 0.0}
    for t in PP.DISTANCE_THRESHOLDS:
        assert s["within[{!r}]".format(t)] == {"median": 1.0, "p95": 1.0, "max": 1.0}
    assert s["gt_common"] == 2 and s["gt_only_a"] == s["gt_only_b"] == 0
    assert s["d_overlap_src"]["max"] == 0.0 and s["d_overlap_tgt"]["max"] == 0.0
    assert [(e["scene"], e["sample"]) for e in rep["clouds"]] == [(i, k) for i in range(SCENES) for k in (0, 1)]
    assert sorted(s["by_sample"]) == ["0", "1"] and all(p["identical_clouds"] == p["compared"] == SCENES for p in s["by_sample"].values())
    for e in rep["clouds"]:
        assert e["n_a"] == e["n_b"] == len(scene_clouds(e["scene"])[e["sample"]]) and e["hausdorff"] == 0.0


def test_a_known_shift_is_the_chamfer_and_the_hausdorff_distance(trees):
    """Every point's nearest neighbour in the shifted tree is its own copy, 3/64 away (the grid spacing is 8/64)."""
    rep = compare_datasets(trees["a"], trees["shifted"], 0, SCENES, backend="numpy-spec")
    s = rep["summary"]
    assert s["identical"] is False and s["compared"] == 2 * SCENES
    for e in rep["clouds"]:
        assert e["chamfer"] == SHIFT_LEN and e["hausdorff"] == SHIFT_LEN and e["p50"] == SHIFT_LEN and e["p99"] == SHIFT_LEN
        assert e["within"] == {"0.0001": 0.0, "0.001": 0.0, "0.0125": 0.0, "0.0375": 0.0}
    assert s["chamfer"] == {"median": SHIFT_LEN, "p95": SHIFT_LEN, "max": SHIFT_LEN}
    assert s["hausdorff"]["max"] == SHIFT_LEN
    for k in ("0", "1"):                                                 # the same per sample index
        part = s["by_sample"][k]
        assert part["compared"] == SCENES and part["identical_clouds"] == 0 and part["chamfer"]["median"] == SHIFT_LEN
        assert part["within[0.0375]"] == {"median": 0.0, "p95": 0.0, "max": 0.0, "min": 0.0}
    rep = compare_datasets(trees["a"], trees["shifted"], 0, SCENES, backend="numpy-spec", thresholds=(0.04, SHIFT_LEN))
    assert all(e["within"] == {"0.04": 0.0, "0.046875": 1.0} for e in rep["clouds"])


def test_a_missing_file_is_counted_and_not_aggregated(trees):
    rep = compare_datasets(trees["a"], trees["holes"], 0, SCENES, backend="numpy-spec")
    s = rep["summary"]
    assert s["missing_a"] == 0 and s["missing_b"] == 1 and s["compared"] == 2 * SCENES - 1 and s["identical"] is True
    entry, = [e for e in rep["clouds"] if e["missing_b"]]
    assert (entry["scene"], entry["sample"]) == (1, 1) and "chamfer" not in entry and "n_a" not in entry
    rep = compare_datasets(trees["holes"], trees["shifted"], 0, SCENES, backend="numpy-spec")
    assert rep["summary"]["missing_a"] == 1 and rep["summary"]["missing_b"] == 0
    assert rep["summary"]["chamfer"]["median"] == SHIFT_LEN and rep["summary"]["compared"] == 2 * SCENES - 1
    # scenes outside [start, stop) are not looked at; a launch boundary in the middle changes nothing
    rep2 = compare_datasets(trees["holes"], trees["shifted"], 0, SCENES, backend="numpy-spec", scenes_per_launch=1)
    assert rep2 == rep
    assert compare_datasets(trees["a"], trees["holes"], 0, 1, backend="numpy-spec")["summary"]["missing_b"] == 0
    # nothing compared is not "identical"
    s = compare_datasets(trees["a"], trees["base"] / "nowhere", 0, SCENES, backend="numpy-spec")["summary"]
    assert s["compared"] == 0 and s["missing_b"] == 2 * SCENES and s["identical"] is False and np.isnan(s["chamfer"]["max"])


def test_gt_log_lines(trees):
    """A has metadata/gt.log, the other trees only their scenes' files: scene 0's line is in both, scene 1's only in A,
    scene 2's only in B."""
    assert read_gt(trees["a"], 0, SCENES) == {(0, 0, 1): (0.5, 0.625), (1, 0, 1): (0.75, 0.875)}
    assert read_gt(trees["a"], 1, SCENES) == {(1, 0, 1): (0.75, 0.875)}
    assert read_gt(trees["shifted"], 0, SCENES) == {(0, 0, 1): (0.4375, 0.6875), (2, 0, 1): (0.25, 0.125)}
    rep = compare_datasets(trees["a"], trees["shifted"], 0, SCENES, backend="numpy-spec")
    assert rep["gt"]["common"] == 1 and rep["gt"]["only_a"] == 1 and rep["gt"]["only_b"] == 1
    assert rep["gt"]["lines"] == [{"scene": 0, "s": 0, "t": 1, "d_overlap_src": 0.0625, "d_overlap_tgt": 0.0625}]
    s = rep["summary"]
    assert (s["gt_common"], s["gt_only_a"], s["gt_only_b"]) == (1, 1, 1)
    assert s["d_overlap_src"] == {"median": 0.0625, "p95": 0.0625, "max": 0.0625} and s["d_overlap_tgt"]["max"] == 0.0625


def test_bad_backend(trees):
    with pytest.raises(ValueError):
        compare_datasets(trees["a"], trees["same"], 0, 1, backend="auto")


def test_cli_writes_the_json_it_prints(trees, tmp_path):
    out = tmp_path / "report.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "compare_datasets.py"), str(trees["a"]), str(trees["shifted"]),
                        "-start", "0", "-stop", str(SCENES), "--backend", "numpy-spec", "--out", str(out)],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    printed = json.loads(r.stdout.strip().splitlines()[-1])
    report = json.loads(out.read_text())
    assert printed == report["summary"] and printed["chamfer"]["median"] == SHIFT_LEN and printed["identical"] is False
    want = compare_datasets(trees["a"], trees["shifted"], 0, SCENES, backend="numpy-spec")
    assert report == json.loads(json.dumps(want))


# ---- on the GPU ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("other", ["same", "shifted", "holes"])
def test_hip_backend_gives_the_numpy_report(trees, other):
    spec = compare_datasets(trees["a"], trees[other], 0, SCENES, backend="numpy-spec")
    hip = compare_datasets(trees["a"], trees[other], 0, SCENES, backend="hip")
    assert hip.pop("backend") == "hip" and spec.pop("backend") == "numpy-spec"
    assert hip == spec                                       # == on every float (no NaN in these reports)
    hip1 = compare_datasets(trees["a"], trees[other], 0, SCENES, backend="hip", scenes_per_launch=2)
    hip1.pop("backend")
    assert hip1 == spec


S, DIM, STEPS, BATCH, SEED = 32, 16, 8, 3, 11


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """The same three synthetic scenes generated twice in fp32 and once in bf16 through the package API."""
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.unet import MaskUnet, Unet
    base = tmp_path_factory.mktemp("generated")
    for name, dtype in (("fp32", "fp32"), ("fp32_again", "fp32"), ("bf16", "bf16")):
        net = Unet(DIM, dtype=dtype).init_synthetic(3)
        mask = MaskUnet(DIM, dtype=dtype).init_synthetic(4, final_bias=8.0)
        diff = GaussianDiffusion(net, image_size=S, timesteps=1000, sampling_timesteps=STEPS)
        gen = Generator(diff, None, batch_size=BATCH, samples_folder=str(base / name / "data"), synthetic_seed=SEED)
        gen.generate(0, SCENES, 1, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, gt_log=True)
        diff.close(); net.close(); mask.close()
    return base


@pytest.mark.gpu
def test_two_fp32_runs_compare_as_identical(generated):
    rep = compare_datasets(generated / "fp32", generated / "fp32_again", 0, SCENES)
    s = rep["summary"]
    assert rep["backend"] == "hip" and s["identical"] is True and s["compared"] == 2 * SCENES
    assert s["missing_a"] == s["missing_b"] == 0 and s["hausdorff"]["max"] == 0.0
    assert s["gt_only_a"] == s["gt_only_b"] == 0 and (s["gt_common"] == 0 or s["d_overlap_src"]["max"] == 0.0)


@pytest.mark.gpu
def test_an_fp32_and_a_bf16_run_are_both_in_the_report(generated):
    """No distance is asserted for bf16: that is what tools/dataset_equivalence.py measures."""
    rep = compare_datasets(generated / "fp32", generated / "bf16", 0, SCENES)
    s = rep["summary"]
    assert s["compared"] == 2 * SCENES and s["missing_a"] == s["missing_b"] == 0
    assert [(e["scene"], e["sample"]) for e in rep["clouds"]] == [(i, k) for i in range(SCENES) for k in (0, 1)]
    for e in rep["clouds"]:
        rel = os.path.join("data", "scene-{:0>6d}".format(e["scene"]), "sample-{:0>6d}.cloud.ply".format(e["sample"]))
        assert e["n_a"] == len(PP.read_ply(str(generated / "fp32" / rel)))
        assert e["n_b"] == len(PP.read_ply(str(generated / "bf16" / rel)))
        if not e["empty"]:
            assert e["hausdorff"] >= e["p99"] >= e["p50"] >= 0.0
