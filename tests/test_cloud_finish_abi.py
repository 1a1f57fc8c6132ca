"""Finishing a cloud on the device, checked without a GPU: the new entry point's header / binding / export, the `gt_log`
keyword and `--with_gt` flag, and the numpy specification `postprocess.finish_cloud` against the bytes the C++ writer pool
puts into a PLY (the same comparison `geometry.finish_clouds` has to pass on the GPU, tests/test_gpu_cloud_finish.py)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pointreggpt_amd import _lib
from pointreggpt_amd import postprocess as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "prg_rigid_crop_ragged_f64"


def test_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert NAME in set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    assert NAME in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == 12
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), NAME)


def test_generate_has_gt_log_off_by_default():
    from pointreggpt_amd.generator import Generator
    assert inspect.signature(Generator.generate).parameters["gt_log"].default is False


def test_cli_lists_with_gt():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_dataset.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--with_gt" in r.stdout


def test_cpu_generator_refuses_gt_log(tmp_path):
    from pointreggpt_amd.generator import Generator

    class _Diff:
        image_size = 16

    gen = Generator(_Diff(), None, samples_folder=str(tmp_path / "out"), synthetic_seed=1, device="cpu")
    with pytest.raises(ValueError, match="gt_log"):
        gen.generate(0, 1, 1, gt_log=True)
    assert not any((tmp_path / "out").iterdir())          # refused before anything was produced


# ---- postprocess.finish_cloud == the vertex payload of WriterPool.cloud's PLY ---------------------------------------------
def _pose(rng):
    """A rigid 4x4 with an irrational rotation (every product rounds) as float64 of a float32 matrix, like `poses0[j]`."""
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("XYZ", rng.uniform(-0.3, 0.3, 3)).as_matrix()
    T[:3, 3] = rng.uniform(-0.4, 0.4, 3)
    return T.astype(np.float32).astype(np.float64)


def _cloud(rng, n):
    return rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 4.0], (n, 3))


def _payload(path, n_rows):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert ("element vertex %d\n" % n_rows).encode() in head
    return body


def _cases():
    rng = np.random.RandomState(20240607)
    T = _pose(rng)
    Ti = np.linalg.inv(T)
    out = {}
    out["pre_crop_voxel_post"] = dict(xyz=_cloud(rng, 6000), valid=None, pre=T, crop=True, voxel=0.025, post=Ti)
    out["crop_only"] = dict(xyz=_cloud(rng, 3000), valid=None, pre=None, crop=True, voxel=0, post=None)
    out["voxel_0"] = dict(xyz=_cloud(rng, 2000), valid=None, pre=T, crop=True, voxel=0, post=Ti)
    xyz = _cloud(rng, 4000)
    valid = rng.rand(4000) < 0.6
    xyz[~valid] = np.nan
    xyz[np.flatnonzero(~valid)[::3], 1] = np.inf
    out["mask_with_nan"] = dict(xyz=xyz, valid=valid, pre=T, crop=True, voxel=0.025, post=Ti)
    xyz = _cloud(rng, 500)
    xyz[0], xyz[1], xyz[2] = PP.BBOX_MAX, PP.BBOX_MIN, [1.5, 0.0, np.nextafter(3.5, 4.0)]     # on hi, on lo, one ulp outside
    out["point_on_hi"] = dict(xyz=xyz, valid=None, pre=None, crop=True, voxel=0, post=None)
    xyz = _cloud(rng, 300) * 0.5 + [0, 0, 1.0]
    xyz[::7, 0] = -0.0
    xyz[3::11, 1] = -0.0
    out["minus_zero_no_transform"] = dict(xyz=xyz, valid=None, pre=None, crop=True, voxel=0, post=None)
    out["crop_empties"] = dict(xyz=_cloud(rng, 400) + [0, 0, 10.0], valid=None, pre=T, crop=True, voxel=0.025, post=Ti)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_finish_cloud_is_the_writer_pools_payload(name, tmp_path):
    c = CASES[name]
    want = PP.finish_cloud(c["xyz"], c["valid"], pre=c["pre"], crop=c["crop"], lo=PP.BBOX_MIN, hi=PP.BBOX_MAX, voxel=c["voxel"],
                           post=c["post"])
    assert want.dtype == np.float64 and want.ndim == 2 and want.shape[1] == 3
    path = str(tmp_path / "c.ply")
    with PP.WriterPool(2) as pool:
        pool.cloud(path, c["xyz"], c["valid"], pre=c["pre"], crop=c["crop"], voxel=c["voxel"], post=c["post"])
        pool.wait()
    assert _payload(path, len(want)) == want.astype("<f8").tobytes()
    if name == "crop_empties":
        assert len(want) == 0
    elif name == "point_on_hi":
        rows = {r.tobytes() for r in want}
        assert np.asarray(PP.BBOX_MAX, dtype=np.float64).tobytes() in rows and np.asarray(PP.BBOX_MIN, dtype=np.float64).tobytes() in rows
        assert c["xyz"][2].tobytes() not in rows
    elif name == "minus_zero_no_transform":
        assert np.signbit(want[want[:, 0] == 0, 0]).all() and np.signbit(want[:, 0]).sum() >= 300 // 7
    else:
        assert len(want) > 0
    if c["valid"] is not None:
        assert np.isfinite(want).all()
