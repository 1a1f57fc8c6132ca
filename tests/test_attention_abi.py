"""The attention test hooks' interface, checked without a GPU: header, binding, exported symbols, and every PRG_E_INVALID case —
all of them are rejected before the first device call, with the hook's name in the message, so none needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pointreggpt_amd import _lib
from test_attention_refs import STATIC_LIMIT, block_weights, static_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"prg_debug_attention_core": 8, "prg_debug_layernorm": 8, "prg_debug_linear_attention_block": 15}
PRG_E_INVALID = -1
F32, BF16, MXFP8, F16X3 = _lib.PRG_F32, _lib.PRG_BF16, _lib.PRG_MXFP8, _lib.PRG_F16X3


def test_hooks_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(str(_lib.LIB_PATH))
    for name, n in ARITY.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n, name
        assert name in _lib.PROTOTYPES, name
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == n, name
        assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def host():
    """Host buffers that stand in for device pointers: an invalid call must return before anything looks at them."""
    buf = (C.c_float * 4096)(*[-7.0] * 4096)
    return dict(p=C.cast(buf, C.c_void_p), buf=buf)


def rejected(lib, rc, name):
    return rc == PRG_E_INVALID and name.encode() in lib.prg_last_error()


def untouched(host):
    return all(v == -7.0 for v in host["buf"])


def test_attention_core_rejects_bad_arguments_before_any_device_call(host):
    lib, p = _lib.load(), host["p"]
    good = dict(qkv=p, out=p, B=1, N=128, dtype=BF16, linear=0, kernel=0)
    bad = [dict(qkv=None), dict(out=None), dict(B=0), dict(B=-1), dict(B=65536), dict(N=0), dict(N=-5), dict(B=4096, N=4096),
           dict(dtype=MXFP8), dict(dtype=-1), dict(dtype=4), dict(linear=2), dict(linear=-1), dict(kernel=2), dict(kernel=-1),
           dict(linear=1, dtype=F16X3), dict(linear=1, kernel=1),
           dict(kernel=1, dtype=F32), dict(kernel=1, dtype=F32, N=256),
           dict(kernel=1, dtype=BF16, N=96), dict(kernel=1, dtype=BF16, N=129), dict(kernel=1, dtype=BF16, N=2048),
           dict(kernel=1, dtype=F16X3, N=64), dict(kernel=1, dtype=F16X3, N=1), dict(kernel=1, dtype=F16X3, N=384)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.prg_debug_attention_core(a["qkv"], a["out"], a["B"], a["N"], a["dtype"], a["linear"], a["kernel"], None)
        assert rejected(lib, rc, "prg_debug_attention_core"), change
    assert untouched(host)


def test_layernorm_rejects_bad_arguments_before_any_device_call(host):
    lib, p = _lib.load(), host["p"]
    good = dict(x=p, g=p, res=None, out=p, M=4, C=64, dtype=F32)
    bad = [dict(x=None), dict(g=None), dict(out=None), dict(M=0), dict(M=-1), dict(M=2 ** 31, C=8), dict(C=0), dict(C=-8),
           dict(C=6), dict(C=12, dtype=BF16), dict(C=4, dtype=BF16), dict(C=1028), dict(C=2056, dtype=BF16),
           dict(dtype=F16X3), dict(dtype=MXFP8), dict(dtype=-1)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.prg_debug_layernorm(a["x"], a["g"], a["res"], a["out"], a["M"], a["C"], a["dtype"], None)
        assert rejected(lib, rc, "prg_debug_layernorm"), change
    assert untouched(host)


def test_linear_attention_block_rejects_bad_arguments_before_any_device_call(host):
    lib, p = _lib.load(), host["p"]
    C_ = 64
    W = {k: np.ascontiguousarray(v.numpy(), dtype=np.float32) for k, v in block_weights(C_, 1).items()}
    wp = {k: v.ctypes.data_as(C.c_void_p) for k, v in W.items()}
    used = C.c_int(-7)
    good = dict(x=p, out=p, B=1, C=C_, N=64, dtype=BF16, shift=-1, psum=-1, **wp)
    bad = [dict(x=None), dict(out=None), dict(norm_g=None), dict(w_qkv=None), dict(w_out=None), dict(b_out=None), dict(out_g=None),
           dict(B=0), dict(B=65536), dict(N=0), dict(N=-64), dict(B=4096, N=4096), dict(N=2 ** 21 + 64), dict(dtype=F32), dict(dtype=MXFP8), dict(dtype=7),
           dict(C=32), dict(C=512), dict(C=0), dict(C=96),
           dict(dtype=F16X3, C=256), dict(dtype=F16X3, N=100), dict(dtype=F16X3, N=16),
           dict(dtype=F16X3, shift=0), dict(dtype=F16X3, shift=1), dict(dtype=F16X3, psum=0), dict(dtype=F16X3, psum=1),
           dict(shift=2), dict(shift=-2), dict(psum=2), dict(psum=-2)]

    def call(a):
        return lib.prg_debug_linear_attention_block(a["x"], a["norm_g"], a["w_qkv"], a["w_out"], a["b_out"], a["out_g"], a["out"], a["B"],
                                                    a["C"], a["N"], a["dtype"], a["shift"], a["psum"], C.byref(used), None)
    for change in bad:
        assert rejected(lib, call(dict(good, **change)), "prg_debug_linear_attention_block"), change
    # the static shifts are refused when the bound of the packed weights does not hold (host arithmetic on the weights alone)
    big = block_weights(C_, 1)
    big["w_qkv"][:256] *= 2.0
    assert float(static_bounds(big["w_qkv"], big["norm_g"]).max()) > STATIC_LIMIT
    w2 = np.ascontiguousarray(big["w_qkv"].numpy(), dtype=np.float32)
    assert rejected(lib, call(dict(good, shift=1, w_qkv=w2.ctypes.data_as(C.c_void_p))), "prg_debug_linear_attention_block")
    assert used.value == -7 and untouched(host)
