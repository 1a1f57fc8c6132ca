"""The fine-label interface, checked without a GPU: header, binding, exported symbol, every PRG_E_INVALID case — all of them are
rejected before the first device call, so none needs a device — and the signatures of the Python layers."""
import ctypes as C
import inspect
import os
import re

import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = "prg_patch_corr_labels_f64"
PRG_E_INVALID = -1
P, I, L, D = C.c_void_p, C.c_int, C.c_int64, C.c_double


def test_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(str(_lib.LIB_PATH))
    assert LABELS in declared and LABELS in _lib.PROTOTYPES and hasattr(lib, LABELS)
    assert _lib.PROTOTYPES[LABELS] == (C.c_int, [P, L, P, L, I, P, L, D, P, P])
    assert declared == set(_lib.PROTOTYPES)
    m = re.search(r"int\s+prg_patch_corr_labels_f64\s*\(([^)]*)\)", hdr)
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const double* pts", "int64_t rows", "const int32_t* table", "int64_t nodes", "int limit",
                    "const int32_t* pairs", "int64_t n_sel", "double radius", "uint8_t* labels", "void* stream"]
    assert "finelabels.hip" in open(os.path.join(ROOT, "pointreggpt_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "pointreggpt_amd", "csrc", "finelabels.hip"))
    assert not hasattr(C.CDLL(str(_lib.LIB_PATH.with_name("libprg_cpu.so"))), "prg_cpu_patch_corr_labels_f64")   # no CPU twin


@pytest.fixture(scope="module")
def host():
    """Host buffers that stand in for device pointers: an invalid call must return before anything looks at them."""
    bufs = dict(pts=(C.c_double * 12)(), table=(C.c_int32 * 8)(0, 1, 4, 4, 2, 3, 4, 4), pairs=(C.c_int32 * 2)(0, 1),
                labels=(C.c_uint8 * 25)(*[0xAB] * 25))
    return {k: C.cast(v, C.c_void_p) for k, v in bufs.items()}, bufs, {k: bytes(v) for k, v in bufs.items()}


def call(lib, a):
    return lib.prg_patch_corr_labels_f64(a["pts"], a["rows"], a["table"], a["nodes"], a["limit"], a["pairs"], a["n_sel"],
                                         a["radius"], a["labels"], None)


def test_rejects_bad_arguments_before_any_device_call(host):
    lib = _lib.load()
    ptrs, bufs, before = host
    good = dict(ptrs, rows=4, nodes=2, limit=4, n_sel=1, radius=0.05)
    bad = [dict(pts=None), dict(table=None), dict(pairs=None), dict(labels=None),
           dict(table=None, rows=0, pts=None), dict(labels=None, rows=0, pts=None), dict(pairs=None, rows=0),
           dict(rows=-1), dict(rows=2 ** 31), dict(rows=-1, pts=None), dict(rows=1, pts=None),
           dict(nodes=0), dict(nodes=-1), dict(nodes=2 ** 31),
           dict(limit=0), dict(limit=-1), dict(limit=257), dict(limit=2 ** 20),
           dict(n_sel=0), dict(n_sel=-1), dict(n_sel=2 ** 24 + 1), dict(n_sel=2 ** 40),
           dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan"))]
    for change in bad:
        rc = call(lib, dict(good, **change))
        assert rc == PRG_E_INVALID and LABELS.encode() in lib.prg_last_error(), change
    for k, v in bufs.items():
        assert bytes(v) == before[k], k                               # host buffers untouched, the sentinels included


def test_python_layers_exist_with_the_documented_signatures():
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    empty = inspect.Parameter.empty
    assert list(inspect.signature(PP.patch_corr_labels).parameters)[:4] == ["points", "table", "pairs", "radius"]
    assert list(inspect.signature(G.patch_corr_labels).parameters) == ["points", "table", "pairs", "radius"]
    sig = inspect.signature(PP.patch_corr_labels_hip).parameters
    assert list(sig) == ["points", "table", "pairs", "radius", "device"] and sig["device"].default == "cuda"
    sig = inspect.signature(PP.select_node_corr).parameters
    assert list(sig) == ["overlap", "corr_offsets", "keys", "min_overlap", "num_targets"]
    for name in ("min_overlap", "num_targets"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is empty
    sig = inspect.signature(G.select_node_corr).parameters
    assert list(sig) == ["gt", "min_overlap", "num_targets", "keys", "generator"]
    assert [sig[n].default for n in list(sig)[1:]] == [0.1, 128, None, None]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig)[1:])
    sig = inspect.signature(PP.fine_ground_truth).parameters
    assert list(sig) == ["pyramid", "gt", "fine_level", "radius", "keys", "min_overlap", "num_targets"]
    assert [sig[n].default for n in list(sig)[2:]] == [empty, empty, empty, 0.1, 128]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig)[2:])
    sig = inspect.signature(G.fine_ground_truth).parameters
    assert list(sig) == ["pyr", "gt", "fine_level", "radius", "min_overlap", "num_targets", "keys", "generator"]
    assert [sig[n].default for n in list(sig)[2:]] == [empty, empty, 0.1, 128, None, None]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig)[2:])
    assert "synchronisation" in G.fine_ground_truth.__doc__


def test_python_layers_refuse_host_tensors():
    """No CPU path: a host tensor is an error, not a fallback."""
    import torch

    from pointreggpt_amd import geometry as G
    z = torch.zeros((4, 3), dtype=torch.float64)
    table, pairs = torch.zeros((2, 4), dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32)
    gt = {"overlap": torch.zeros(1, dtype=torch.float64), "corr_offsets": torch.tensor([0, 1]), "table": table,
          "node_corr": pairs}
    with pytest.raises(_lib.PrgError):
        G.patch_corr_labels(z, table, pairs, 0.05)
    with pytest.raises(_lib.PrgError):
        G.select_node_corr(gt)
    with pytest.raises(_lib.PrgError):
        G.fine_ground_truth({"points": [z]}, gt, fine_level=0, radius=0.05)
