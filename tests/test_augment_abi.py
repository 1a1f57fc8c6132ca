"""The augmentation interface, checked without a GPU: header, binding, exported symbol, the new `PairStream` keywords, and every
PRG_E_INVALID case of prg_augment_ragged_f64 — all of them are refused before the first device call, so none needs a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "prg_augment_ragged_f64"
PRG_E_INVALID = -1
P, I, L = C.c_void_p, C.c_int, C.c_int64


def test_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(str(_lib.LIB_PATH))
    assert NAME in declared and NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    res, args = _lib.PROTOTYPES[NAME]
    assert res is C.c_int and len(args) == 16
    assert args == [P, P, I, L, P, P, P, C.c_uint32, P, L, C.c_double, P, L, P, P, P]
    assert declared == set(_lib.PROTOTYPES)
    assert not hasattr(C.CDLL(str(_lib.LIB_PATH.with_name("libprg_cpu.so"))), "prg_cpu_augment_ragged_f64")   # no CPU twin


def test_pair_stream_has_the_new_keywords_off_by_default():
    from pointreggpt_amd.stream import Augment, PairStream
    par = inspect.signature(PairStream.__init__).parameters
    assert par["augment"].default is None and par["epoch"].default == 0
    assert par["augment"].kind is inspect.Parameter.KEYWORD_ONLY and par["epoch"].kind is inspect.Parameter.KEYWORD_ONLY
    a = Augment()
    assert (a.noise, a.point_limit, a.rotation, a.translation) == (0.005, 30000, "src", 1.0)
    for bad in (dict(rotation="tgt"), dict(noise=-1.0), dict(noise=float("nan")), dict(point_limit=0), dict(translation=-1.0)):
        with pytest.raises(ValueError):
            Augment(**bad)


def test_python_layers_exist_with_the_documented_signatures():
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    from pointreggpt_amd import synthetic
    par = inspect.signature(PP.augment_cloud).parameters
    assert list(par)[0] == "points"
    assert {k: par[k].default for k in list(par)[2:]} == dict(draw=0, noise=0.0, limit=None, T=None, keys=None)
    assert par["seed"].default is inspect.Parameter.empty and par["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    par = inspect.signature(G.augment_clouds).parameters
    assert list(par)[:2] == ["points", "lengths"]
    for k, d in dict(draw=0, noise=0.0, limit=None, T=None, has_T=None, keys=None).items():
        assert par[k].default == d and par[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert "none" in G.augment_clouds.__doc__.lower() and "synchronisation" in G.augment_clouds.__doc__
    assert callable(PP.augment_clouds_hip)
    assert list(inspect.signature(synthetic.augment_seed).parameters) == ["base_seed", "scene_index", "cloud"]


def test_python_layer_refuses_host_tensors():
    """No CPU path: a host tensor is an error, not a fallback."""
    import torch
    from pointreggpt_amd import geometry as G
    with pytest.raises(_lib.PrgError):
        G.augment_clouds(torch.zeros((4, 3), dtype=torch.float64), [4], seeds=[1])


@pytest.fixture(scope="module")
def host():
    """Host buffers standing in for device memory: a call that is refused must not touch them (and never launches)."""
    bufs = dict(pts=np.full((8, 3), 7.0), offsets=np.array([0, 3, 8], dtype=np.int64), T=np.tile(np.eye(4), (2, 1, 1)),
                has_T=np.ones(2, dtype=np.uint8), seeds=np.array([1, 2], dtype=np.uint64), keys=np.zeros(8, dtype=np.uint32),
                out_offsets=np.array([0, 3, 8], dtype=np.int64), out=np.full((8, 3), -5.0), rows=np.full(8, -9, dtype=np.int32))
    return bufs, {k: v.tobytes() for k, v in bufs.items()}


def test_rejects_bad_arguments_before_any_device_call(host):
    lib = _lib.load()
    bufs, before = host
    good = dict({k: v.ctypes.data for k, v in bufs.items()}, C=2, total=8, draw=0, limit=0, noise=0.005, out_total=8)

    def call(**change):
        a = dict(good, **change)
        return lib.prg_augment_ragged_f64(a["pts"], a["offsets"], a["C"], a["total"], a["T"], a["has_T"], a["seeds"], a["draw"],
                                          a["keys"], a["limit"], a["noise"], a["out_offsets"], a["out_total"], a["out"], a["rows"],
                                          None)

    bad = [dict(offsets=None), dict(out_offsets=None), dict(seeds=None), dict(C=0), dict(C=-1), dict(C=65536), dict(total=-1),
           dict(total=2 ** 31), dict(out_total=-1), dict(out_total=2 ** 31), dict(limit=-1), dict(noise=-0.5),
           dict(noise=float("nan")), dict(noise=float("inf")), dict(T=None), dict(out=good["pts"]), dict(pts=None),
           dict(out=None), dict(rows=None)]
    for change in bad:
        rc = call(**change)
        assert rc == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), change
    for k, v in bufs.items():
        assert v.tobytes() == before[k], k                            # host buffers untouched, the sentinels included
    # without rows there is nothing to launch and no address to check: fine with null buffers, still no device call
    assert call(total=0, pts=None) == 0 and call(out_total=0, out=None, rows=None) == 0
