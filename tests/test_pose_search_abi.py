"""The pose-search interface, checked without a GPU: headers, bindings, exported symbols, the new keywords, the host-only
workspace arithmetic, and every PRG_E_INVALID case of prg_pose_candidate_counts and its twin — all of them are refused before
the first device call, so none needs a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from pointreggpt_amd import _lib, cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, SIZE, TWIN = "prg_pose_candidate_counts", "prg_pose_candidate_workspace_bytes", "prg_cpu_pose_candidate_counts"
PRG_E_INVALID = -1
P, I, F = C.c_void_p, C.c_int, C.c_float


def declared(header, prefix):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", hdr))


def test_entry_points_are_declared_bound_and_exported():
    names = declared("prg.h", "prg_")
    lib = C.CDLL(str(_lib.LIB_PATH))
    for n in (NAME, SIZE):
        assert n in names and n in _lib.PROTOTYPES and hasattr(lib, n)
    assert _lib.PROTOTYPES[NAME] == (C.c_int, [P, P, P, P, I, I, I, I, P, F, P, P, C.c_size_t, P])
    assert _lib.PROTOTYPES[SIZE] == (C.c_size_t, [I, I, I, I])
    assert names == set(_lib.PROTOTYPES)
    twins = declared("prg_cpu.h", "prg_cpu_")
    assert TWIN in twins and twins == set(cpu.PROTOTYPES) and hasattr(C.CDLL(str(cpu.LIB_PATH)), TWIN)
    assert cpu.PROTOTYPES[TWIN] == (C.c_int, [P, P, P, P, I, I, I, I, P, F, P])        # the same without workspace and stream
    mk = open(os.path.join(ROOT, "pointreggpt_amd", "csrc", "Makefile")).read()
    assert "posesearch.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]
    # the camera arithmetic is written once: both users include the header, neither defines it
    for src in ("geometry.hip", "posesearch.hip"):
        text = open(os.path.join(ROOT, "pointreggpt_amd", "csrc", src)).read()
        assert '#include "camera.h"' in text and "void se3_apply(" not in text and "struct Cam" not in text, src


def test_python_layers_exist_with_the_documented_signatures():
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.stream import PairStream
    assert list(inspect.signature(G.pose_candidates).parameters) == ["seed", "scene", "sample_idx", "n", "spread"]
    assert list(inspect.signature(G.select_pose_candidates).parameters) == ["counts", "rows", "band"]
    par = inspect.signature(G.pose_candidate_counts).parameters
    assert list(par)[:5] == ["pts", "offs", "poses", "K", "S"] and par["box"].default is None and par["z_tol"].default == 0.0375
    assert "none" in G.pose_candidate_counts.__doc__.lower() and "synchronisation" in G.pose_candidate_counts.__doc__
    assert callable(PP.pose_candidate_counts) and callable(PP.pose_candidate_counts_hip) and callable(cpu.ops.pose_candidate_counts)
    for fn in (Generator.generate, PairStream.__init__):
        par = inspect.signature(fn).parameters
        assert (par["overlap"].default, par["pose_candidates"].default, par["pose_spread"].default) == (None, 16, 3.0)
    cli = open(os.path.join(ROOT, "generate_dataset.py")).read()
    assert all(opt in cli for opt in ('"--overlap"', '"--pose_candidates"', '"--pose_spread"'))


def test_python_layer_refuses_host_tensors():
    """No CPU path behind the HIP front-end: a host tensor is an error, not a fallback."""
    import torch
    from pointreggpt_amd import geometry as G
    with pytest.raises(_lib.PrgError):
        G.pose_candidate_counts(torch.zeros((4, 3)), torch.tensor([0, 4]), np.eye(4, dtype=np.float32)[None, None],
                                np.eye(3, dtype=np.float32)[None], 8)


def test_workspace_bytes_is_host_arithmetic():
    size = _lib.load().prg_pose_candidate_workspace_bytes
    assert size(3, 5, 16, 16) == 3 * 5 * 16 * 16 * 4
    assert size(64, 16, 128, 128) == 64 * 16 * 128 * 128 * 4                     # 64 MiB: below the cap
    one = 64 * 256 * 256 * 4                                                     # 16 MiB per candidate
    assert size(64, 32, 256, 256) == 16 * one == 256 << 20                       # capped at 256 MiB, whole candidates
    assert size(64, 16, 256, 256) == 16 * one
    assert size(7, 1000, 300, 300) == ((256 << 20) // (7 * 300 * 300 * 4)) * 7 * 300 * 300 * 4
    assert size(65535, 2, 128, 128) == 65535 * 128 * 128 * 4                     # never less than one candidate per scene
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -3)):
        assert size(*bad) == 0


@pytest.fixture(scope="module")
def host():
    """Host buffers standing in for device memory: a call that is refused must not touch them (and never launches)."""
    bufs = dict(points=np.full((8, 3), 2.0, dtype=np.float32), offsets=np.array([0, 3, 8], dtype=np.int64),
                poses=np.tile(np.eye(4, dtype=np.float32), (2, 3, 1, 1)), K=np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)),
                box=np.array([-1, -1, 0, 1, 1, 4], dtype=np.float32), counts=np.full((2, 3, 3), -9, dtype=np.int32),
                workspace=np.full(2 * 3 * 4 * 4, 0x5A5A5A5A, dtype=np.uint32))
    return bufs, {k: v.tobytes() for k, v in bufs.items()}


BAD = [dict(points=None), dict(offsets=None), dict(poses=None), dict(K=None), dict(counts=None), dict(workspace=None),
       dict(B=0), dict(B=-1), dict(B=65536), dict(N=0), dict(N=-2), dict(N=65536), dict(H=0), dict(W=0), dict(H=-4), dict(W=-1),
       dict(H=65536, W=65536), dict(z_tol=-0.01), dict(z_tol=float("nan")), dict(z_tol=float("inf"))]


def test_rejects_bad_arguments_before_any_device_call(host):
    lib = _lib.load()
    bufs, before = host
    good = dict({k: v.ctypes.data for k, v in bufs.items()}, B=2, N=3, H=4, W=4, z_tol=0.0375, workspace_bytes=2 * 3 * 4 * 4 * 4)

    def call(**change):
        a = dict(good, **change)
        return lib.prg_pose_candidate_counts(a["points"], a["offsets"], a["poses"], a["K"], a["B"], a["N"], a["H"], a["W"], a["box"],
                                             a["z_tol"], a["counts"], a["workspace"], a["workspace_bytes"], None)

    small = [dict(workspace_bytes=0), dict(workspace_bytes=2 * 4 * 4 * 4 - 1),       # less than one candidate per scene
             dict(workspace=good["workspace"] + 1)]                                  # not a 32-bit address
    for change in BAD + small:
        rc = call(**change)
        assert rc == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), change
    for k, v in bufs.items():
        assert v.tobytes() == before[k], k                                           # host buffers untouched, the sentinels included


def test_twin_rejects_the_same_arguments(host):
    lib = cpu.load()
    bufs, before = host
    good = dict({k: v.ctypes.data for k, v in bufs.items()}, B=2, N=3, H=4, W=4, z_tol=0.0375)

    def call(**change):
        a = dict(good, **change)
        return lib.prg_cpu_pose_candidate_counts(a["points"], a["offsets"], a["poses"], a["K"], a["B"], a["N"], a["H"], a["W"],
                                                 a["box"], a["z_tol"], a["counts"])

    for change in BAD:
        if "workspace" in change:
            continue
        assert call(**change) == PRG_E_INVALID and TWIN.encode() in lib.prg_cpu_last_error(), change
    for k, v in bufs.items():
        assert v.tobytes() == before[k], k
    assert call() == 0                                                               # and the good call runs: the twin is host code
    assert bufs["counts"].tolist() == [[[3, 0, 1]] * 3, [[5, 0, 1]] * 3]             # K = identity: every row (2, 2, 2) in pixel (1, 1),
    assert call(box=None) == 0                                                       # outside the box
    assert bufs["counts"].tolist() == [[[3, 3, 1]] * 3, [[5, 5, 1]] * 3]
