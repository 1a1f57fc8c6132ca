"""The device voxel grid's interface, checked without a GPU: header, binding, exported symbols, the host-only workspace
arithmetic, and the backend keywords of the three callers."""
import ctypes
import inspect
import os
import re

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("prg_voxel_grid_workspace_bytes", "prg_voxel_grid_ragged", "prg_merge_memory_f64")


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert _lib.PROTOTYPES["prg_voxel_grid_workspace_bytes"][0] is ctypes.c_size_t
    assert len(_lib.PROTOTYPES["prg_voxel_grid_ragged"][1]) == 12
    assert len(_lib.PROTOTYPES["prg_merge_memory_f64"][1]) == 11


def test_workspace_bytes_is_host_arithmetic():
    """Callable without a device; > 0 for total > 0; non-decreasing in total and in B; fine for total = 0."""
    f = _lib.load().prg_voxel_grid_workspace_bytes
    assert f(0, 1) >= 0 and f(0, 64) >= 0
    totals = [0, 1, 2, 255, 256, 1023, 1024, 1025, 4096, 100_000, 1_000_000, 2_000_000, 20_000_000, 2 ** 31 - 1]
    segs = [1, 2, 3, 16, 64, 65, 512, 1024, 2048, 65535]
    for B in segs:
        sizes = [f(t, B) for t in totals]
        assert all(s > 0 for s, t in zip(sizes, totals) if t > 0), (B, sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (B, sizes)
    for t in totals:
        sizes = [f(t, B) for B in segs]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (t, sizes)
    # keys and row indices, each double-buffered for the sort: at least 24 bytes per row
    assert f(1_000_000, 1) >= 24 * 1_000_000


def test_backend_keywords_and_defaults():
    from pointreggpt_amd import postprocess as PP
    from pointreggpt_amd.generator import Generator, generate_gt
    from pointreggpt_amd.tester import Tester
    assert inspect.signature(Generator.generate).parameters["voxel_backend"].default == "device"
    assert inspect.signature(Tester.generate).parameters["voxel_backend"].default == "device"
    assert inspect.signature(PP.overlap_ratios_hip).parameters["voxel"].default == "device"
    assert inspect.signature(generate_gt).parameters["voxel"].default == "device"
