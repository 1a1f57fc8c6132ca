"""The conv-selection hook (prg_debug_conv_choice), checked without a GPU: header, binding, exported symbol, and every
PRG_E_INVALID case with the hook's name in the message.  The hook makes no device call at all; tests/test_conv_dispatch.py pins
what it answers."""
import ctypes as C
import os
import re

from pointreggpt_amd import _lib
from test_conv_dispatch import CC, Hook, Q, SWITCHES, conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "prg_debug_conv_choice"
PRG_E_INVALID = -1


def test_hook_is_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prg.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr)
    assert m, NAME
    assert [" ".join(a.split()[:-1]) for a in m.group(1).split(",")] == ["const int32_t*", "const int32_t*", "int32_t*", "float*"]
    res, args = _lib.PROTOTYPES[NAME]
    assert res is C.c_int and args == [C.c_void_p] * 4
    assert hasattr(C.CDLL(str(_lib.LIB_PATH)), NAME)
    assert re.search(rf"PRG_CQ_COUNT = PRG_CQ_SWITCHES \+ {len(SWITCHES)}\b", hdr) and len(Q) + len(SWITCHES) == 36


def test_rejects_bad_arguments():
    hook = Hook(256, {})
    lib = hook.lib
    good = conv("bf16", 2, 64, 64, 64, 64, bias=1)
    out, scale = (C.c_int32 * len(CC))(*[-7] * len(CC)), C.c_float(-7.0)

    def call(q, q2=None, o=out, s=C.byref(scale)):
        return lib.prg_debug_conv_choice(hook.array(q) if q else None, hook.array(q2) if q2 else None, o, s)
    assert call(good) == 0 and out[0] != -7
    out[:] = [-7] * len(CC)
    scale.value = -7.0
    bad = [dict(dtype=4), dict(dtype=-1),                                     # bad dtype
           dict(C0=60), dict(C0=68), dict(C1=4), dict(C0=0), dict(C0=-64),     # C0 / C1 % the 16-byte vector (bf16: 8 elements)
           dict(CoutPad=0), dict(Cout=128), dict(CoutPad=96), dict(Cout=65),   # CoutPad < Cout, or not a multiple of 64
           dict(B=0), dict(B=-1), dict(Hin=0), dict(Win=-4), dict(Hout=0), dict(Wout=0), dict(Cout=0), dict(KH=0), dict(KW=-3),
           dict(stride=0), dict(pad=-1), dict(kchunks=0), dict(ups=2), dict(B=65536, Hout=256, Wout=256),   # M >= 2^31
           dict(present=-1), dict(present=1 << 15)]
    for change in bad:
        for q, q2 in ((dict(good, **change), None), (good, dict(good, **change))):
            assert call(q, q2) == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), (change, lib.prg_last_error())
    for args in ((None, None, out, C.byref(scale)), (good, None, None, C.byref(scale)), (good, None, out, None)):
        assert call(*args) == PRG_E_INVALID and NAME.encode() in lib.prg_last_error()
    assert list(out) == [-7] * len(CC) and scale.value == -7.0               # a rejected call writes nothing
    f32 = conv("fp32", 2, 64, 64, 64, 64, bias=1)
    assert call(dict(f32, C0=60)) == 0 and call(dict(f32, C0=62)) == PRG_E_INVALID             # float storage: 4 elements
