"""The radius-pairs interface, checked without a GPU: header, binding, exported symbols, the host-only workspace arithmetic, and
every PRG_E_INVALID case — all of them are rejected before the first device call, so none needs a device."""
import ctypes as C
import inspect
import os
import re

import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("prg_radius_pairs_workspace_bytes", "prg_radius_count_ragged_f64", "prg_radius_fill_ragged_f64")
PRG_E_INVALID = -1
INF, NAN = float("inf"), float("nan")


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert _lib.PROTOTYPES["prg_radius_pairs_workspace_bytes"] == (C.c_size_t, [C.c_int64])
    assert len(_lib.PROTOTYPES["prg_radius_count_ragged_f64"][1]) == 10
    assert len(_lib.PROTOTYPES["prg_radius_fill_ragged_f64"][1]) == 9


def test_workspace_bytes_is_host_arithmetic():
    f = _lib.load().prg_radius_pairs_workspace_bytes
    totals = [0, 1, 2, 255, 256, 1023, 1024, 1025, 4096, 100_000, 1_000_000, 20_000_000, 2 ** 31 - 1]
    sizes = [f(t) for t in totals]
    assert all(s > 0 for s in sizes), sizes
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] > sizes[0]


@pytest.fixture(scope="module")
def host():
    """Host buffers that stand in for device pointers: an invalid call must return before anything looks at them."""
    pts = (C.c_double * 12)()
    offs = (C.c_int64 * 3)(0, 2, 4)
    row_start = (C.c_int64 * 5)(*[-7] * 5)
    corr = (C.c_int32 * 16)(*[-7] * 16)
    ws = (C.c_char * 4096)()
    p = lambda b: C.cast(b, C.c_void_p)          # noqa: E731
    return dict(pts=p(pts), offs=p(offs), row_start=p(row_start), corr=p(corr), ws=p(ws), keep=(pts, offs, row_start, corr, ws),
                row_start_buf=row_start, corr_buf=corr)


def rejected(lib, rc, name):
    return rc == PRG_E_INVALID and name.encode() in lib.prg_last_error()


def test_count_rejects_bad_arguments_before_any_device_call(host):
    lib = _lib.load()
    h = host
    need = lib.prg_radius_pairs_workspace_bytes(4)
    good = dict(pts=h["pts"], offs=h["offs"], n_pairs=1, total=4, max_cloud=2, radius=0.5, row_start=h["row_start"], ws=h["ws"],
                ws_bytes=4096)
    assert need <= 4096
    bad = [dict(pts=None), dict(offs=None), dict(row_start=None), dict(ws=None),
           dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=65536),
           dict(radius=0.0), dict(radius=-1.0), dict(radius=INF), dict(radius=-INF), dict(radius=NAN),
           dict(ws_bytes=0), dict(ws_bytes=need - 1),
           dict(total=-1), dict(total=2 ** 31), dict(max_cloud=0), dict(max_cloud=2 ** 31)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.prg_radius_count_ragged_f64(a["pts"], a["offs"], a["n_pairs"], a["total"], a["max_cloud"], a["radius"],
                                             a["row_start"], a["ws"], a["ws_bytes"], None)
        assert rejected(lib, rc, "prg_radius_count_ragged_f64"), change
    # a workspace sized for fewer rows than `total`
    big = 10_000_000
    assert lib.prg_radius_pairs_workspace_bytes(big) > 4096
    rc = lib.prg_radius_count_ragged_f64(h["pts"], h["offs"], 1, big, 2, 0.5, h["row_start"], h["ws"], 4096, None)
    assert rejected(lib, rc, "prg_radius_count_ragged_f64")
    assert list(h["row_start_buf"]) == [-7] * 5                      # nothing was written


def test_fill_rejects_bad_arguments_before_any_device_call(host):
    lib = _lib.load()
    h = host
    good = dict(pts=h["pts"], offs=h["offs"], n_pairs=1, max_cloud=2, radius=0.5, row_start=h["row_start"], capacity=8,
                corr=h["corr"])
    bad = [dict(pts=None), dict(offs=None), dict(row_start=None), dict(corr=None),
           dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=65536),
           dict(radius=0.0), dict(radius=-1.0), dict(radius=INF), dict(radius=NAN),
           dict(capacity=-1), dict(max_cloud=0), dict(max_cloud=2 ** 31)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.prg_radius_fill_ragged_f64(a["pts"], a["offs"], a["n_pairs"], a["max_cloud"], a["radius"], a["row_start"],
                                            a["capacity"], a["corr"], None)
        assert rejected(lib, rc, "prg_radius_fill_ragged_f64"), change
    assert list(h["corr_buf"]) == [-7] * 16


def test_python_layers_exist_with_the_documented_signatures():
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    from pointreggpt_amd.stream import PairStream
    assert list(inspect.signature(PP.radius_pairs).parameters) == ["a", "b", "radius", "chunk"]
    assert inspect.signature(PP.radius_pairs).parameters["chunk"].default == 1024
    assert list(inspect.signature(PP.radius_pairs_hip).parameters) == ["pairs", "radius", "device"]
    assert list(inspect.signature(G.radius_pairs_ragged).parameters) == ["pts", "offsets", "n_pairs", "max_cloud", "radius"]
    sig = inspect.signature(PairStream.__init__).parameters
    assert list(sig)[1:3] == ["generator", "depth_correction"]
    for name, default in (("matching_radius", None), ("mask_threshold", 0.99), ("has_refine_step", False),
                          ("save_voxel_size", 0.025), ("to", "numpy")):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    for name in ("start", "stop", "noise_seed"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is inspect.Parameter.empty, name
