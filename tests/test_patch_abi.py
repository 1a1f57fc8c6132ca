"""The patch-table interface, checked without a GPU: header, binding, exported symbols, every PRG_E_INVALID case — all of them
are rejected before the first device call, so none needs a device — and the signatures of the Python layers."""
import ctypes as C
import inspect
import os
import re

import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES, OVERLAP = "prg_patch_tables_ragged", "prg_patch_overlap_ragged_f64"
PRG_E_INVALID = -1
P, I, L, D = C.c_void_p, C.c_int, C.c_int64, C.c_double


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(str(_lib.LIB_PATH))
    for name in (TABLES, OVERLAP):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert _lib.PROTOTYPES[TABLES] == (C.c_int, [P, P, P, I, L, L, I, P, P, P, P, P, P])
    assert _lib.PROTOTYPES[OVERLAP] == (C.c_int, [P, P, I, P, P, L, I, D, P, L, L, P, P, P])
    assert "patches.hip" in open(os.path.join(ROOT, "pointreggpt_amd", "csrc", "Makefile")).read()


def test_every_declared_entry_point_is_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(str(_lib.LIB_PATH))
    assert declared == set(_lib.PROTOTYPES)
    assert [name for name in sorted(declared) if not hasattr(lib, name)] == []


@pytest.fixture(scope="module")
def host():
    """Host buffers that stand in for device pointers: an invalid call must return before anything looks at them."""
    bufs = dict(d2=(C.c_double * 6)(), assign=(C.c_int32 * 6)(0, 1, 0, 0, 0, 0), offs=(C.c_int64 * 3)(0, 4, 6),
                t_offs=(C.c_int64 * 3)(0, 2, 4), base=(C.c_int32 * 2)(0, 0), pad=(C.c_int32 * 2)(4, 4),
                table=(C.c_int32 * 16)(*[-7] * 16), sizes=(C.c_int32 * 4)(*[-7] * 4), pts=(C.c_double * 18)(),
                h_offs=(C.c_int64 * 2)(0, 4), boxes=(C.c_double * 24)(*[-7.0] * 24), hits=(C.c_int32 * 8)(*[-7] * 8))
    return {k: C.cast(v, C.c_void_p) for k, v in bufs.items()}, bufs, {k: bytes(v) for k, v in bufs.items()}


def call_tables(lib, a):
    return lib.prg_patch_tables_ragged(a["d2"], a["assign"], a["offs"], a["n_pairs"], a["max_cloud"], a["max_nodes"], a["limit"],
                                       a["t_offs"], a["base"], a["pad"], a["table"], a["sizes"], None)


def call_overlap(lib, a):
    return lib.prg_patch_overlap_ragged_f64(a["pts"], a["offs"], a["n_pairs"], a["table"], a["t_offs"], a["max_nodes"], a["limit"],
                                            a["radius"], a["h_offs"], a["total"], a["max_item"], a["boxes"], a["hits"], None)


def rejected(lib, call, name, good, bad):
    for change in bad:
        rc = call(lib, dict(good, **change))
        assert rc == PRG_E_INVALID and name.encode() in lib.prg_last_error(), change


def test_tables_rejects_bad_arguments_before_any_device_call(host):
    lib = _lib.load()
    ptrs, bufs, before = host
    good = dict(ptrs, n_pairs=1, max_cloud=4, max_nodes=2, limit=4)
    rejected(lib, call_tables, TABLES, good,
             [dict(d2=None), dict(assign=None), dict(offs=None), dict(t_offs=None), dict(table=None), dict(sizes=None),
              dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=65536),
              dict(max_cloud=0), dict(max_cloud=-1), dict(max_cloud=2 ** 31), dict(max_nodes=0), dict(max_nodes=2 ** 31),
              dict(limit=0), dict(limit=-1), dict(limit=257), dict(limit=2 ** 20),
              # every check holds whether index_base / pad are given or null
              dict(base=None, limit=0), dict(pad=None, n_pairs=0), dict(base=None, pad=None, table=None)])
    for k, v in bufs.items():
        assert bytes(v) == before[k], k                               # host buffers untouched, the sentinels included


def test_overlap_rejects_bad_arguments_before_any_device_call(host):
    lib = _lib.load()
    ptrs, bufs, before = host
    good = dict(ptrs, n_pairs=1, max_nodes=2, limit=4, radius=0.05, total=4, max_item=4)
    rejected(lib, call_overlap, OVERLAP, good,
             [dict(pts=None), dict(offs=None), dict(table=None), dict(t_offs=None), dict(h_offs=None), dict(hits=None),
              dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=65536),
              dict(max_nodes=0), dict(max_nodes=-1), dict(max_nodes=2 ** 31),
              dict(limit=0), dict(limit=-1), dict(limit=257), dict(limit=2 ** 20),
              dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")),
              dict(total=0), dict(total=-1), dict(total=2 ** 28 + 1, max_item=4), dict(total=2 ** 31, max_item=2 ** 31),
              dict(max_item=0), dict(max_item=5),
              dict(boxes=None, limit=0), dict(boxes=None, hits=None)])      # ... whether the pre-filter's scratch is given or not
    for k, v in bufs.items():
        assert bytes(v) == before[k], k


def test_python_layers_exist_with_the_documented_signatures():
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    assert list(inspect.signature(PP.node_patches).parameters) == ["points", "nodes", "limit"]
    assert list(inspect.signature(PP.patch_overlaps).parameters)[:5] == ["src_points", "src_table", "tgt_points", "tgt_table", "radius"]
    sig = inspect.signature(G.node_patches_ragged).parameters
    assert list(sig) == ["points", "point_offsets", "nodes", "node_offsets", "limit", "index_base", "pad"]
    assert sig["index_base"].default is None and sig["pad"].default is None
    for fn in (PP.coarse_ground_truth, G.coarse_ground_truth):
        sig = inspect.signature(fn).parameters
        assert list(sig) == [list(sig)[0], "fine_level", "limit", "radius"]
        for name in ("fine_level", "limit", "radius"):
            assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is inspect.Parameter.empty, name
    assert callable(PP.node_patches_hip) and callable(PP.patch_overlaps_hip) and callable(G.patch_overlaps_ragged)


def test_python_layers_refuse_host_tensors():
    """No CPU path: a host tensor is an error, not a fallback."""
    import torch

    from pointreggpt_amd import geometry as G
    z = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(_lib.PrgError):
        G.node_patches_ragged(z, [0, 4], z[:2], [0, 2], 4)
    with pytest.raises(_lib.PrgError):
        G.patch_overlaps_ragged(z, [0, 2, 4], torch.zeros((2, 4), dtype=torch.int32), [0, 1, 2], 0.05)
    with pytest.raises(_lib.PrgError):
        G.coarse_ground_truth({"points": [z], "lengths": [torch.tensor([2, 2])]}, fine_level=0, limit=4, radius=0.05)
