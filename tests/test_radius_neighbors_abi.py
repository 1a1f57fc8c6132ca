"""The neighbour-table interface, checked without a GPU: header, binding, exported symbol, every PRG_E_INVALID case — all of them
are rejected before the first device call, so none needs a device — and the signatures of the Python layers."""
import ctypes as C
import inspect
import os
import re

import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "prg_radius_select_ragged_f64"
PRG_E_INVALID = -1


def test_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(str(_lib.LIB_PATH))
    assert NAME in declared and NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    res, args = _lib.PROTOTYPES[NAME]
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    assert res is C.c_int and args == [P, P, I, L, P, P, L, I, P, P, P, P, P]
    assert "neighbors.hip" in open(os.path.join(ROOT, "pointreggpt_amd", "csrc", "Makefile")).read()


@pytest.fixture(scope="module")
def host():
    """Host buffers that stand in for device pointers: an invalid call must return before anything looks at them."""
    pts = (C.c_double * 12)()
    offs = (C.c_int64 * 3)(0, 2, 4)
    row_start = (C.c_int64 * 5)(0, 1, 2, 2, 2)
    corr = (C.c_int32 * 4)(0, 0, 1, 1)
    t_offs = (C.c_int64 * 2)(0, 2)
    base = (C.c_int32 * 1)(0)
    pad = (C.c_int32 * 1)(2)
    table = (C.c_int32 * 16)(*[-7] * 16)
    p = lambda b: C.cast(b, C.c_void_p)          # noqa: E731
    bufs = dict(pts=pts, offs=offs, row_start=row_start, corr=corr, t_offs=t_offs, base=base, pad=pad, table=table)
    return {k: p(v) for k, v in bufs.items()}, bufs, {k: bytes(v) for k, v in bufs.items()}


def call(lib, a):
    return lib.prg_radius_select_ragged_f64(a["pts"], a["offs"], a["n_pairs"], a["max_cloud"], a["row_start"], a["corr"],
                                            a["list_rows"], a["limit"], a["t_offs"], a["base"], a["pad"], a["table"], None)


def test_select_rejects_bad_arguments_before_any_device_call(host):
    lib = _lib.load()
    ptrs, bufs, before = host
    good = dict(ptrs, n_pairs=1, max_cloud=2, list_rows=2, limit=4)
    bad = [dict(pts=None), dict(offs=None), dict(row_start=None), dict(t_offs=None), dict(table=None),
           dict(corr=None),                                           # a list with rows needs its corr
           dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=65536),
           dict(max_cloud=0), dict(max_cloud=-1), dict(max_cloud=2 ** 31),
           dict(list_rows=-1), dict(list_rows=-1, corr=None),
           dict(limit=0), dict(limit=-1), dict(limit=1025), dict(limit=2 ** 20)]
    for change in bad:
        rc = call(lib, dict(good, **change))
        assert rc == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), change
    # every check holds whether index_base / pad are given or null
    for change in (dict(base=None, limit=0), dict(pad=None, n_pairs=0), dict(base=None, pad=None, table=None)):
        rc = call(lib, dict(good, **change))
        assert rc == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), change
    for k, v in bufs.items():
        assert bytes(v) == before[k], k                               # host buffers untouched, the table's sentinel included


def test_python_layers_exist_with_the_documented_signatures():
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    assert list(inspect.signature(PP.radius_neighbors).parameters) == ["a", "b", "radius", "limit"]
    assert list(inspect.signature(PP.neighbor_pyramid).parameters) == ["points", "lengths", "num_stages", "voxel_size", "radius",
                                                                       "neighbor_limits"]
    assert list(inspect.signature(PP.radius_neighbors_hip).parameters) == ["pairs", "radius", "limit", "device"]
    sig = inspect.signature(G.radius_neighbors_ragged).parameters
    assert list(sig) == ["pts", "offsets", "n_pairs", "max_cloud", "radius", "limit", "index_base", "pad"]
    assert sig["index_base"].default is None and sig["pad"].default is None
    sig = inspect.signature(G.neighbor_pyramid).parameters
    assert list(sig) == ["points", "lengths", "num_stages", "voxel_size", "radius", "neighbor_limits"]
    for name in ("num_stages", "voxel_size", "radius", "neighbor_limits"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is inspect.Parameter.empty, name


def test_python_layers_refuse_host_tensors():
    """No CPU path: a host tensor is an error, not a fallback."""
    import torch

    from pointreggpt_amd import geometry as G
    with pytest.raises(_lib.PrgError):
        G.radius_neighbors_ragged(torch.zeros((4, 3), dtype=torch.float64), torch.tensor([0, 2, 4]), 1, 2, 0.5, 4)
    with pytest.raises(_lib.PrgError):
        G.neighbor_pyramid(torch.zeros((4, 3), dtype=torch.float64), [4], num_stages=1, voxel_size=0.025, radius=0.0625,
                           neighbor_limits=[4])
