"""The fused ResnetBlock tail's test hook (prg_debug_resblock_tail), checked without a GPU: header, binding, exported symbol, and
every PRG_E_INVALID case: all of them are rejected before the first device call, with the hook's name in the message, so none
needs a device."""
import ctypes as C
import os
import re

import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "prg_debug_resblock_tail"
ARITY = 18
PRG_E_INVALID = -1


def test_hook_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr)
    assert m, NAME
    assert len(m.group(1).split(",")) == ARITY
    res, args = _lib.PROTOTYPES[NAME]
    assert res is C.c_int and len(args) == ARITY
    assert hasattr(C.CDLL(str(_lib.LIB_PATH)), NAME)


@pytest.fixture(scope="module")
def host():
    """Host buffers that stand in for device pointers: an invalid call must return before anything looks at them."""
    buf = (C.c_float * 4096)(*[-7.0] * 4096)
    return dict(p=C.cast(buf, C.c_void_p), buf=buf)


def test_rejects_bad_arguments_before_any_device_call(host):
    lib, p = _lib.load(), host["p"]
    good = dict(h=p, s0=p, s1=p, A=p, Bc=p, w_res=p, b_res=p, head_w=None, head_b=None, out=p, B=1, N=64, C0=64, C1=64, Cout=64,
                sig=0, in_place=0)
    bad = [dict(h=None), dict(s0=None), dict(s1=None), dict(A=None), dict(Bc=None), dict(w_res=None), dict(b_res=None), dict(out=None),
           dict(head_w=p), dict(head_b=p),                                         # the head's weight and bias come together
           dict(B=0), dict(B=-1), dict(B=65536), dict(N=0), dict(N=-64), dict(B=4096, N=4096), dict(B=3, N=2 ** 31 - 1),
           dict(C0=0, C1=128), dict(C0=128, C1=0), dict(C0=-64, C1=192), dict(C0=60, C1=68), dict(C0=64, C1=32), dict(C0=32, C1=32),
           dict(Cout=128), dict(Cout=32), dict(Cout=0), dict(C0=128, C1=64, Cout=64), dict(C0=128, C1=128, Cout=64),
           dict(C0=128, C1=128, Cout=256), dict(C0=256, C1=256, Cout=128),
           dict(head_w=p, head_b=p, C0=128, C1=64, Cout=128), dict(head_w=p, head_b=p, C0=128, C1=128, Cout=128),
           dict(sig=2), dict(sig=-1), dict(in_place=2), dict(in_place=-1)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.prg_debug_resblock_tail(a["h"], a["s0"], a["s1"], a["A"], a["Bc"], a["w_res"], a["b_res"], a["head_w"], a["head_b"],
                                         a["out"], a["B"], a["N"], a["C0"], a["C1"], a["Cout"], a["sig"], a["in_place"], None)
        assert rc == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), change
    assert all(v == -7.0 for v in host["buf"])
