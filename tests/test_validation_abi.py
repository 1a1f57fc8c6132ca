"""The validation entries, checked without a GPU: header, binding, exported symbols, the workspace size, and every PRG_E_INVALID
case of prg_q_sample / prg_diffusion_loss / prg_mask_metrics -- all refused before the first device call, so none needs a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prg_validate_workspace_bytes", "prg_q_sample", "prg_diffusion_loss", "prg_mask_metrics")
PRG_E_INVALID = -1
P, I, F, U32, SZ = C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.c_size_t


def header():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def params(hdr, name):
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        ident = p.split("*")[-1].split()[-1]
        out.append((p[:len(p) - len(ident)].strip(), ident))
    return out


def ctype_of(decl):
    return P if decl.endswith("*") else {"int": I, "float": F, "uint32_t": U32, "size_t": SZ}[decl]


def test_entries_are_declared_bound_and_exported():
    hdr = header()
    declared = set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
        res, args = _lib.PROTOTYPES[name]
        assert [ctype_of(t) for t, _n in params(hdr, name)] == args, name
        assert res is (SZ if name == NAMES[0] else C.c_int)
    assert declared == set(_lib.PROTOTYPES)
    assert [n for _t, n in params(hdr, "prg_q_sample")] == ["x0", "a", "s", "noise", "seeds", "draw", "B", "HW", "x_t", "noise_out", "stream"]
    assert [n for _t, n in params(hdr, "prg_diffusion_loss")] == ["u", "x0", "noise", "seeds", "draw", "a", "s", "w", "objective", "loss_type",
                                                                  "B", "HW", "workspace", "workspace_bytes", "out", "stream"]
    assert [n for _t, n in params(hdr, "prg_mask_metrics")] == ["prob", "input", "label", "mask", "threshold", "tol", "B", "HW", "workspace",
                                                                "workspace_bytes", "counts", "sums", "stream"]
    assert _lib.load().prg_abi_version() == 1


def test_stream_tags_are_distinct_ascii_words():
    src = open(os.path.join(ROOT, "pointreggpt_amd", "csrc", "sampler.h")).read()
    tags = {k: int(v, 16) for k, v in re.findall(r"PHILOX_DOMAIN_(\w+) = (0x[0-9A-Fa-f]+)u", src)}
    from pointreggpt_amd import validate as V
    assert tags == {"NORMAL": 0x70726721, "KEEP": 0x6B656570, "VALIDATE": V.TAG_NOISE}
    for tag in (V.TAG_NOISE, V.TAG_TIMESTEP):
        assert all(0x20 <= b < 0x7F for b in tag.to_bytes(4, "big"))
    assert len({V.TAG_NOISE, V.TAG_TIMESTEP, 0x70726721, 0x6B656570, 0x6175676D}) == 5


def test_workspace_bytes():
    lib = _lib.load()
    ws = lib.prg_validate_workspace_bytes
    assert ws(1, 1) == ws(1, 4096) == 24 and ws(1, 4097) == 48 and ws(3, 4100) == 3 * 48 and ws(64, 1 << 24) == 64 * 4096 * 24
    for B, HW in ((0, 4), (-1, 4), (1, 0), (1, -4), (65536, 4), (1, (1 << 30) + 1)):
        assert ws(B, HW) == 0


def test_python_layer():
    from pointreggpt_amd import validate as V
    from pointreggpt_amd.diffusion import GaussianDiffusion
    par = inspect.signature(GaussianDiffusion.__init__).parameters
    assert par["min_snr_loss_weight"].default is False and par["min_snr_gamma"].default == 5 and par["loss_type"].default == "l1"
    par = inspect.signature(GaussianDiffusion.q_sample).parameters
    assert list(par) == ["self", "x_start", "t", "noise", "seeds", "draw"] and par["seeds"].kind is inspect.Parameter.KEYWORD_ONLY
    par = inspect.signature(GaussianDiffusion.p_losses).parameters
    assert list(par) == ["self", "x_start", "t", "param_cond", "noise", "seeds", "draw", "per_sample"]
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("noise", "seeds", "draw", "per_sample"))
    assert callable(GaussianDiffusion.forward)
    import torch
    with pytest.raises(_lib.PrgError):                 # no quiet host path behind the device front-ends
        V.q_sample_hip(torch.zeros((1, 4)), torch.ones(1), torch.ones(1), torch.zeros((1, 4)))


@pytest.fixture(scope="module")
def host():
    """Host buffers standing in for device memory: a refused call must not touch them (and never launches)."""
    bufs = dict(x=np.full((2, 8), 7.0, dtype=np.float32), y=np.full((2, 8), -5.0, dtype=np.float32), c=np.ones(2, dtype=np.float32),
                seeds=np.array([1, 2], dtype=np.uint64), ws=np.full(16, -3.0), out=np.full((2, 4), -9.0), counts=np.full((2, 4), -9, dtype=np.int64))
    return bufs, {k: v.tobytes() for k, v in bufs.items()}


def test_bad_arguments_are_refused_before_any_device_call(host):
    lib = _lib.load()
    bufs, before = host
    a = {k: v.ctypes.data for k, v in bufs.items()}
    big = 1 << 20

    def q_sample(**ch):
        k = dict(dict(x0=a["x"], a=a["c"], s=a["c"], noise=a["x"], seeds=None, draw=0, B=2, HW=8, x_t=a["y"], noise_out=None), **ch)
        return lib.prg_q_sample(k["x0"], k["a"], k["s"], k["noise"], k["seeds"], k["draw"], k["B"], k["HW"], k["x_t"], k["noise_out"], None)

    def loss(**ch):
        k = dict(dict(u=a["x"], x0=a["x"], noise=a["x"], seeds=None, draw=0, a=a["c"], s=a["c"], w=a["c"], objective=2, loss_type=0, B=2, HW=8,
                      ws=a["ws"], nbytes=big, out=a["out"]), **ch)
        return lib.prg_diffusion_loss(k["u"], k["x0"], k["noise"], k["seeds"], k["draw"], k["a"], k["s"], k["w"], k["objective"],
                                      k["loss_type"], k["B"], k["HW"], k["ws"], k["nbytes"], k["out"], None)

    def metrics(**ch):
        k = dict(dict(prob=a["x"], input=a["x"], label=a["x"], mask=None, thr=0.5, tol=0.005, B=2, HW=8, ws=a["ws"], nbytes=big,
                      counts=a["counts"], sums=a["out"]), **ch)
        return lib.prg_mask_metrics(k["prob"], k["input"], k["label"], k["mask"], k["thr"], k["tol"], k["B"], k["HW"], k["ws"], k["nbytes"],
                                    k["counts"], k["sums"], None)

    shape = [dict(B=0), dict(B=-1), dict(B=65536), dict(HW=0), dict(HW=-8), dict(HW=(1 << 30) + 4)]
    noise = [dict(noise=None, seeds=None), dict(noise=a["x"], seeds=a["seeds"]), dict(noise=None, seeds=a["seeds"], HW=6)]
    cases = [(q_sample, b"prg_q_sample", shape + noise + [dict(x0=None), dict(a=None), dict(s=None), dict(x_t=None)]),
             (loss, b"prg_diffusion_loss", shape + noise + [dict(u=None), dict(x0=None), dict(a=None), dict(s=None), dict(w=None), dict(ws=None),
                                                            dict(out=None), dict(objective=-1), dict(objective=3), dict(loss_type=-1),
                                                            dict(loss_type=2), dict(nbytes=0), dict(nbytes=47)]),
             (metrics, b"prg_mask_metrics", shape + [dict(prob=None), dict(input=None), dict(label=None), dict(ws=None), dict(counts=None),
                                                     dict(sums=None), dict(nbytes=0), dict(nbytes=47)])]
    for fn, name, bad in cases:
        for change in bad:
            assert fn(**change) == PRG_E_INVALID and name in lib.prg_last_error(), (name, change)
    for k, v in bufs.items():
        assert v.tobytes() == before[k], k
