"""Per-view clouds (`Generator.generate(clouds="per_view")`) and the indexed overlap interface, checked without a GPU: header,
binding, exported symbol, every PRG_E_INVALID case of prg_overlap_counts_indexed — all rejected before the first device call —,
the per-pair augmentation keys, and the `device="cpu"` generator at the configuration of tests/test_gpu_cloud_finish.py (S = 64,
dim 16, 4 DDIM steps of 1000, batches of 2, fp32 synthetic weights, `mask_threshold=0.5`, synthetic seed = noise seed = 11) over
2 scenes.  File comparisons are byte for byte, cloud comparisons bit for bit."""
import ctypes as C
import inspect
import os
import re
from itertools import combinations

import numpy as np
import pytest

from pointreggpt_amd import _lib, synthetic
from pointreggpt_amd import postprocess as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "prg_overlap_counts_indexed"
PRG_E_INVALID = -1
S, DIM, STEPS, BATCH, SCENES = 64, 16, 4, 2, 2
SEED = 11


# ---- the interface -----------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(str(_lib.LIB_PATH))
    assert NAME in declared and NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    P, I, L, D = C.c_void_p, C.c_int, C.c_int64, C.c_double
    assert _lib.PROTOTYPES[NAME] == (C.c_int, [P, P, I, P, I, L, D, P, P])
    assert _lib.PROTOTYPES["prg_overlap_counts"] == (C.c_int, [P, P, I, L, D, P, P])            # the adjacent form is as it was
    assert declared == set(_lib.PROTOTYPES)


def test_indexed_counts_reject_bad_arguments_before_any_device_call():
    """Host buffers stand in for the device pointers: an invalid call must return before anything looks at them."""
    lib = _lib.load()
    bufs = dict(pts=(C.c_double * 12)(), offs=(C.c_int64 * 3)(0, 2, 4), index=(C.c_int32 * 2)(0, 1), counts=(C.c_int32 * 2)(-7, -7))
    before = {k: bytes(v) for k, v in bufs.items()}
    good = dict({k: C.cast(v, C.c_void_p) for k, v in bufs.items()}, n_clouds=2, n_pairs=1, max_cloud=2, radius=0.5)
    bad = [dict(pts=None), dict(offs=None), dict(index=None), dict(counts=None),
           dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=65536),
           dict(n_clouds=0), dict(n_clouds=-3),
           dict(max_cloud=0), dict(max_cloud=-1),
           dict(radius=0.0), dict(radius=-0.5), dict(radius=float("nan"))]
    for change in bad:
        a = dict(good, **change)
        rc = lib.prg_overlap_counts_indexed(a["pts"], a["offs"], a["n_clouds"], a["index"], a["n_pairs"], a["max_cloud"], a["radius"],
                                            a["counts"], None)
        assert rc == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), change
    for k, v in bufs.items():
        assert bytes(v) == before[k], k                               # untouched, the counts' sentinel included


def test_python_layers_exist_with_the_documented_signatures():
    import torch

    from pointreggpt_amd import geometry as G
    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.stream import PairStream, augment_poses
    assert list(inspect.signature(G.overlap_counts_indexed).parameters) == ["pts", "offsets", "pair_index", "max_cloud", "radius"]
    par = inspect.signature(PP.overlap_ratios_indexed_hip).parameters
    assert list(par)[:5] == ["clouds", "pairs", "voxel_size", "overlap_factor", "voxel"]
    assert (par["voxel_size"].default, par["overlap_factor"].default, par["voxel"].default) == (0.025, 1.5, "device")
    assert inspect.signature(Generator.generate).parameters["clouds"].default == "fused"
    par = inspect.signature(PairStream.__init__).parameters
    assert par["num_samples"].default == 1 and par["clouds"].default == "fused"
    assert list(inspect.signature(Generator._pair_ratios.__func__).parameters) == ["cls", "offs", "d_offs", "cnt", "j"]
    assert inspect.signature(augment_poses).parameters["pair"].default is None
    with pytest.raises(_lib.PrgError):                                # no CPU path: a host tensor is an error, not a fallback
        G.overlap_counts_indexed(torch.zeros((4, 3), dtype=torch.float64), torch.tensor([0, 2, 4]),
                                 torch.tensor([[0, 1]], dtype=torch.int32), 2, 0.5)


def test_pair_ratios_is_the_general_form_at_adjacent_segments():
    from pointreggpt_amd.generator import Generator
    offs = np.array([0, 1500, 2600, 3700, 5000, 5900, 7000])           # 3 clouds per scene, 2 scenes; cloud 4 is too small
    d_offs = np.array([0, 100, 300, 600, 1000, 1000, 1500])
    cnt = np.array([[50, 150], [5, 10], [30, 400]])
    assert Generator._pair_ratios(offs, d_offs, cnt, 0) == Generator._pair_ratios_at(offs, d_offs, cnt[0], 0, 1) == ((0.5, 0.75), None)
    assert Generator._pair_ratios(offs, d_offs, cnt, 1) == Generator._pair_ratios_at(offs, d_offs, cnt[1], 2, 3)
    assert Generator._pair_ratios(offs, d_offs, cnt, 1)[0] is None     # both ratios below 0.1
    assert Generator._pair_ratios_at(offs, d_offs, cnt[2], 0, 2) == ((0.3, 400 / 300), None)
    r, why = Generator._pair_ratios_at(offs, d_offs, cnt[0], 3, 4)
    assert r is None and "1000" in why


# ---- the augmentation keys of a pair --------------------------------------------------------------------------------------------
def test_augment_seed_per_pair():
    b, s = 11, 5
    for c in (0, 1, 2):
        assert synthetic.augment_seed(b, s, c) == synthetic.augment_seed_pair(b, s, c, pair=(0, 1)) == synthetic.augment_seed_pair(b, s, c, pair=None)
        assert synthetic.augment_seed(b, s, c) == synthetic.augment_seed_pair(b, s, c)
    assert list(inspect.signature(synthetic.augment_seed_pair).parameters) == ["base_seed", "scene_index", "cloud", "pair"]
    keys = [synthetic.augment_seed_pair(b, s, c, pair=p) for c in (0, 1, 2) for p in (None, (0, 2), (1, 2), (2, 1))]
    assert len(set(keys)) == len(keys)
    tag = 0x6175676D
    assert synthetic.augment_seed_pair(b, s, 0, pair=(1, 2)) == int(np.random.SeedSequence([b, s, tag, 1, 2]).generate_state(1, np.uint64)[0])
    assert synthetic.augment_seed_pair(b, s, 2, pair=(0, 2)) == int(np.random.SeedSequence([b, s, tag, 2, 0, 2]).generate_state(1, np.uint64)[0])


def test_augment_poses_per_pair():
    from pointreggpt_amd.stream import Augment, augment_poses
    aug = Augment(rotation="both")
    base = augment_poses(11, 3, 2, aug)
    for same in (None, (0, 1)):
        assert all(np.array_equal(a, b) for a, b in zip(augment_poses(11, 3, 2, aug, pair=same), base))
    t02, t12 = augment_poses(11, 3, 2, aug, pair=(0, 2))[2], augment_poses(11, 3, 2, aug, pair=(1, 2))[2]
    assert not np.array_equal(t02, base[2]) and not np.array_equal(t12, base[2]) and not np.array_equal(t02, t12)


# ---- the generator on the CPU ----------------------------------------------------------------------------------------------------
def tree(root):
    out = {}
    for d, _dirs, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def nets():
    from pointreggpt_amd import cpu
    unet = cpu.Unet(DIM).init_synthetic(3)
    mask = cpu.MaskUnet(DIM).init_synthetic(4, final_bias=8.0)
    return cpu.GaussianDiffusion(unet, image_size=S, timesteps=1000, sampling_timesteps=STEPS), mask


def run(nets, folder, num_samples, clouds, **kw):
    from pointreggpt_amd.generator import Generator
    diff, mask = nets
    gen = Generator(diff, None, batch_size=BATCH, samples_folder=str(folder / "ds" / "data"), synthetic_seed=SEED, device="cpu")
    gen.generate(0, SCENES, num_samples, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, clouds=clouds, **kw)
    return gen


def test_one_view_per_scene_is_the_fused_dataset(nets, tmp_path):
    run(nets, tmp_path / "fused", 1, "fused")
    run(nets, tmp_path / "per_view", 1, "per_view")
    a, b = tree(str(tmp_path / "fused")), tree(str(tmp_path / "per_view"))
    assert sorted(a) == sorted(b) and len(a) == SCENES * 9
    for name in a:
        assert a[name] == b[name], name


@pytest.fixture(scope="module")
def two_views(nets, tmp_path_factory):
    """num_samples = 2 in both modes; the per-view run with every (xyz, valid) of `unproject_f64` and every `_poses` recorded."""
    from pointreggpt_amd import cpu
    from pointreggpt_amd.generator import Generator
    base = tmp_path_factory.mktemp("two_views")
    run(nets, base / "fused", 2, "fused")
    seen = dict(views=[], poses=[])
    real_unproject, real_poses = cpu.ops.unproject_f64, Generator._poses

    def unproject(depth, intrinsic, pose, **kw):
        xyz, valid = real_unproject(depth, intrinsic, pose, **kw)
        if pose is not None:                                           # (the source frames are unprojected without a pose)
            seen["views"].append((xyz.numpy().copy(), valid.numpy().copy()))
        return xyz, valid

    def poses(self, idxs, sample_idx, pose_seed=None):
        out = real_poses(self, idxs, sample_idx, pose_seed)
        seen["poses"].append((list(idxs), sample_idx, out.copy()))
        return out

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(cpu.ops, "unproject_f64", staticmethod(unproject))
        mp.setattr(Generator, "_poses", poses)
        run(nets, base / "per_view", 2, "per_view")
    return tree(str(base / "fused")), tree(str(base / "per_view")), seen, base


def test_two_views_differ_from_fused_in_the_view_clouds_only(two_views):
    a, b, _seen, _ = two_views
    extra = {"ds/data/scene-{:0>6d}/sample-000002.cloud.ply".format(i) for i in range(SCENES)}
    assert set(b) - set(a) == extra and set(a) <= set(b)
    for name in a:
        if not name.endswith(".cloud.ply") or name.endswith("sample-000000.cloud.ply"):
            assert a[name] == b[name], name
    assert any(a[n] != b[n] for n in a if n.endswith("sample-000001.cloud.ply"))         # fused holds both views, per view one


def test_view_clouds_are_finish_cloud_of_the_view_alone(two_views):
    _a, _b, seen, base = two_views
    assert len(seen["views"]) == len(seen["poses"]) == 2               # one batch of 2 scenes, 2 views
    for (idxs, sample_idx, pose), (xyz, valid) in zip(seen["poses"], seen["views"]):
        for j, idx in enumerate(idxs):
            T = pose[j].astype(np.float64)
            want = PP.finish_cloud(xyz[j][valid[j]], pre=T, crop=True, lo=PP.BBOX_MIN, hi=PP.BBOX_MAX, voxel=0.025, post=np.linalg.inv(T))
            got = PP.read_ply(str(base / "per_view" / "ds" / "data" / "scene-{:0>6d}".format(idx) /
                                  "sample-{:0>6d}.cloud.ply".format(sample_idx + 1)))
            assert len(want) >= 1000 and got.shape == want.shape
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (idx, sample_idx)


def test_generate_gt_lists_the_pairs_in_combinations_order(two_views):
    """Seed 11 leaves every one of the three candidate pairs of both scenes in the log on this path (numpy specification of the
    overlap): asserted below, so the order check cannot pass on empty logs."""
    from pointreggpt_amd.generator import generate_gt
    _a, _b, _seen, base = two_views
    generate_gt("ds", 0, SCENES, 3, root=str(base / "per_view"), overlap="numpy-spec")
    order = list(combinations(range(3), 2))
    for i in range(SCENES):
        sdir = base / "per_view" / "ds" / "data" / "scene-{:0>6d}".format(i)
        lines = [ln.split("\t") for ln in (sdir / "gt.log").read_text().splitlines()]
        got = [(int(s), int(t)) for _n, s, t, _o1, _o2 in lines]
        assert got == [p for p in order if p in got] and len(set(got)) == len(got)
        assert (0, 1) in got and any(s >= 1 for s, _t in got)
        for name, s, t, o1, o2 in lines:
            assert name == "scene-{:0>6d}".format(i)
            clouds = [PP.read_ply(str(sdir / "sample-{:0>6d}.cloud.ply".format(k))) for k in (int(s), int(t))]
            assert [o1, o2] == ["{:.4f}".format(r) for r in PP.compute_overlap_ratio(*clouds)]
        for s, t in set(order) - set(got):                                # a missing pair is one the filter drops
            clouds = [PP.read_ply(str(sdir / "sample-{:0>6d}.cloud.ply".format(k))) for k in (s, t)]
            r = PP.compute_overlap_ratio(*clouds)
            assert min(len(c) for c in clouds) < 1000 or np.isnan(r).any() or max(r) < 0.1


def test_bad_clouds_mode(nets, tmp_path):
    with pytest.raises(ValueError):
        run(nets, tmp_path, 1, "nonsense")
    assert not (tmp_path / "ds" / "data" / "scene-000000").exists()        # refused before anything is written
    with pytest.raises(ValueError):
        run(nets, tmp_path, 1, "per_view", gt_log=True)                     # the device finish needs a HIP device, as before


def test_cli_clouds_flag(tmp_path):
    """`generate_dataset.py --device cpu --num_samples 2 --clouds per_view` writes the files of `generate(clouds="per_view")`."""
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "generate_dataset.py"), "--device", "cpu", "--resume", "synthetic:3", "--synthetic", str(SEED),
           "--image_size", str(S), "--sampling_timesteps", str(STEPS), "--batch_size", "1", "--dim", str(DIM), "--mask_threshold", "0.5",
           "--dataset_name", "ds", "-start", "0", "-stop", "1", "--num_samples", "2"]
    r = subprocess.run(cmd + ["--clouds", "per_view"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    sdir = tmp_path / "ds" / "data" / "scene-000000"
    sizes = [len(PP.read_ply(str(sdir / "sample-{:0>6d}.cloud.ply".format(k)))) for k in (0, 1, 2)]
    assert min(sizes) >= 1000
    r = subprocess.run(cmd + ["--clouds", "both"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--clouds" in r.stderr
