"""The normals interface, checked without a GPU: header, binding, exported symbol, every PRG_E_INVALID case — all of them are
rejected before the first device call, so none needs a device — and the signatures of the Python layers."""
import ctypes as C
import inspect
import os
import re

import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "prg_normals_ragged_f64"
PRG_E_INVALID = -1


def test_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(str(_lib.LIB_PATH))
    assert NAME in declared and NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    assert declared == set(_lib.PROTOTYPES)
    res, args = _lib.PROTOTYPES[NAME]
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    # pts, offsets, C, table, table_offsets, pad, count, Q, limit, viewpoints, min_neighbors, normals, variation, scatter, stream
    assert res is C.c_int and args == [P, P, I, P, P, P, P, L, I, P, I, P, P, P, P]
    decl = re.search(NAME + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
    names = [re.sub(r"[\s*]", " ", a).split()[-1] for a in decl.split(",")]
    assert names == ["pts", "offsets", "C", "table", "table_offsets", "pad", "count", "Q", "limit", "viewpoints", "min_neighbors",
                     "normals", "variation", "scatter", "stream"]
    assert "normals.hip" in open(os.path.join(ROOT, "pointreggpt_amd", "csrc", "Makefile")).read()


@pytest.fixture(scope="module")
def host():
    """Host buffers that stand in for device pointers: an invalid call must return before anything looks at them."""
    bufs = dict(pts=(C.c_double * 12)(*range(12)), offs=(C.c_int64 * 3)(0, 2, 4), table=(C.c_int32 * 16)(*[1] * 16),
                t_offs=(C.c_int64 * 3)(0, 2, 4), pad=(C.c_int32 * 2)(4, 4), count=(C.c_int32 * 4)(4, 4, 4, 4),
                views=(C.c_double * 6)(), normals=(C.c_double * 12)(*[-7.0] * 12), variation=(C.c_double * 4)(*[-7.0] * 4),
                scatter=(C.c_double * 24)(*[-7.0] * 24))
    return {k: C.cast(v, C.c_void_p) for k, v in bufs.items()}, bufs, {k: bytes(v) for k, v in bufs.items()}


def call(lib, a):
    return lib.prg_normals_ragged_f64(a["pts"], a["offs"], a["C"], a["table"], a["t_offs"], a["pad"], a["count"], a["Q"], a["limit"],
                                      a["views"], a["min_neighbors"], a["normals"], a["variation"], a["scatter"], None)


def test_rejects_bad_arguments_before_any_device_call(host):
    lib = _lib.load()
    ptrs, bufs, before = host
    good = dict(ptrs, C=2, Q=4, limit=4, min_neighbors=3)
    bad = [dict(pts=None), dict(offs=None), dict(table=None), dict(t_offs=None), dict(count=None), dict(views=None),
           dict(normals=None),
           dict(C=0), dict(C=-1), dict(C=65536),
           dict(limit=0), dict(limit=-1), dict(limit=1025), dict(limit=2 ** 20),
           dict(min_neighbors=2), dict(min_neighbors=0), dict(min_neighbors=-3),
           dict(Q=-1), dict(Q=2 ** 31),
           dict(normals=ptrs["pts"]), dict(variation=ptrs["pts"]), dict(scatter=ptrs["pts"])]
    for change in bad:
        rc = call(lib, dict(good, **change))
        assert rc == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), change
    # every check holds whether the optional pointers are given or null
    for change in (dict(pad=None, limit=0), dict(variation=None, C=0), dict(scatter=None, variation=None, normals=None),
                   dict(pad=None, variation=None, scatter=None, min_neighbors=2)):
        rc = call(lib, dict(good, **change))
        assert rc == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), change
    for k, v in bufs.items():
        assert bytes(v) == before[k], k                               # host buffers untouched, the outputs' sentinels included


def test_no_rows_is_no_launch():
    lib = _lib.load()
    none = dict(pts=None, offs=None, table=None, t_offs=None, pad=None, count=None, views=None, normals=None, variation=None,
                scatter=None)
    assert call(lib, dict(none, C=1, Q=0, limit=30, min_neighbors=3)) == 0
    assert call(lib, dict(none, C=1, Q=0, limit=0, min_neighbors=3)) == PRG_E_INVALID       # ... but the checks still hold


def test_python_layers_exist_with_the_documented_signatures():
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    from pointreggpt_amd import stream as S
    KW, EMPTY = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    sig = inspect.signature(PP.estimate_normals).parameters
    assert list(sig)[:5] == ["points", "table", "count", "viewpoint", "min_neighbors"]
    assert sig["viewpoint"].kind is KW and tuple(sig["viewpoint"].default) == (0, 0, 0) and sig["min_neighbors"].default == 3
    assert all(name.startswith("_") for name in list(sig)[5:])                         # test hooks only
    sig = inspect.signature(PP.estimate_normals_cloud).parameters
    assert list(sig) == ["points", "radius", "limit", "viewpoint", "min_neighbors"]
    assert (sig["radius"].default, sig["limit"].default) == (0.1, 30)
    sig = inspect.signature(PP.estimate_normals_hip).parameters
    assert list(sig) == ["clouds", "radius", "limit", "viewpoints", "device"] and sig["viewpoints"].default is None
    sig = inspect.signature(G.estimate_normals).parameters
    assert list(sig) == ["points", "lengths", "radius", "limit", "viewpoints", "min_neighbors", "want_variation"]
    assert [sig[n].default for n in list(sig)[2:]] == [0.1, 30, None, 3, False]
    assert all(sig[n].kind is KW for n in list(sig)[2:])
    sig = inspect.signature(G.normals_from_tables).parameters
    assert list(sig)[:4] == ["points", "lengths", "table", "count"] and all(sig[n].kind is KW for n in list(sig)[4:])
    assert sig["viewpoints"].default is None and sig["min_neighbors"].default == 3 and sig["want_variation"].default is False
    sig = inspect.signature(S.PairStream.__init__).parameters
    assert sig["normals"].kind is KW and sig["normals"].default is None
    assert list(sig)[-1] == "normals"                                 # appended: no existing keyword moved
    n = S.Normals()
    assert (n.radius, n.limit) == (0.1, 30)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(limit=2),
                dict(limit=1025), dict(limit=3.5)):
        with pytest.raises(ValueError):
            S.Normals(**bad)
    S.Normals(radius=0.05, limit=3), S.Normals(limit=1024)
    with pytest.raises(ValueError):
        PP.estimate_normals([[0.0, 0.0, 0.0]], [[0]], [1], min_neighbors=2)


def test_python_layers_refuse_host_tensors():
    """No CPU path: a host tensor is an error, not a fallback."""
    import torch

    from pointreggpt_amd import geometry as G
    pts = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(_lib.PrgError):
        G.estimate_normals(pts, [4])
    with pytest.raises(_lib.PrgError):
        G.normals_from_tables(pts, [4], torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4,), dtype=torch.int32))
