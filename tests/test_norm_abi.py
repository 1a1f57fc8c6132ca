"""The test hooks of the GroupNorm passes and the conditioning kernels (prg_debug_gn_stats, prg_debug_gn_coeff, prg_debug_gn_fold,
prg_debug_affine_silu, prg_debug_linear, prg_debug_sinusoidal), checked without a GPU: header, binding, exported symbol, the
argument struct's layout against the header, and every PRG_E_INVALID case: all of them are rejected before the first device call,
with the hook's name in the message, so none needs a device."""
import ctypes as C
import os
import re

import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRG_E_INVALID = -1
ARITY = {"prg_debug_gn_stats": 9, "prg_debug_gn_coeff": 19, "prg_debug_gn_fold": 2, "prg_debug_affine_silu": 11, "prg_debug_linear": 16,
         "prg_debug_sinusoidal": 7}
CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int64_t*": C.c_void_p, "int64_t*": C.c_void_p,
         "const int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32}


def header():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


@pytest.mark.parametrize("name", list(ARITY))
def test_hook_is_declared_bound_and_exported(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header())
    assert m, name
    assert len(m.group(1).split(",")) == ARITY[name]
    res, args = _lib.PROTOTYPES[name]
    assert res is C.c_int and len(args) == ARITY[name]
    assert hasattr(C.CDLL(str(_lib.LIB_PATH)), name)


def test_struct_layout_matches_the_header():
    m = re.search(r"typedef struct prg_gn_fold \{(.*?)\} prg_gn_fold;", header(), flags=re.S)
    assert m, "struct prg_gn_fold"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        t = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl)
        assert t and t.group(1) in CTYPE, decl
        fields += [(n.strip(), CTYPE[t.group(1)]) for n in t.group(2).split(",")]
    assert [(n, t) for n, t in _lib.GnFoldC._fields_] == fields
    off = 0
    for name, t in fields:
        size = C.sizeof(t)
        off = (off + size - 1) // size * size
        assert getattr(_lib.GnFoldC, name).offset == off, name
        off += size
    assert C.sizeof(_lib.GnFoldC) == (off + 7) // 8 * 8 == 15 * 8 + 7 * 8 + 10 * 4
    for value, n in enumerate(("NONE", "TABLES", "APPLY")):
        assert re.search(rf"PRG_GF_{n} = {value}\b", header()) and getattr(_lib, f"GF_{n}") == value


@pytest.fixture(scope="module")
def host():
    """Host buffers that stand in for device pointers: an invalid call must return before anything looks at them."""
    buf = (C.c_float * 4096)(*[-7.0] * 4096)
    return dict(p=C.cast(buf, C.c_void_p).value, buf=buf)


def rejected(lib, rc, name, change):
    assert rc == PRG_E_INVALID and name.encode() in lib.prg_last_error(), (name, change, rc, lib.prg_last_error())


def sweep(lib, name, call, good, bad):
    for change in bad:
        rejected(lib, call(dict(good, **change)), name, change)
    return len(bad)


def test_gn_stats_rejects_bad_arguments(host):
    lib, p = _lib.load(), host["p"]
    ns = C.c_int(-5)
    good = dict(x=p, slabs=p, ns=C.byref(ns), B=2, C=64, HW=100, G=8, dtype=_lib.PRG_BF16)
    bad = [dict(x=None), dict(slabs=None), dict(ns=None), dict(dtype=_lib.PRG_MXFP8), dict(dtype=_lib.PRG_F16X3), dict(dtype=-1),
           dict(C=0), dict(C=-8), dict(C=12), dict(C=24), dict(C=4096), dict(C=4), dict(C=12, dtype=_lib.PRG_F32), dict(C=2048, dtype=_lib.PRG_F32),
           dict(G=0), dict(G=-1), dict(G=7), dict(G=128, C=1024), dict(B=0), dict(B=65536), dict(HW=0), dict(HW=-4), dict(B=64, HW=1 << 20)]
    sweep(lib, "prg_debug_gn_stats", lambda a: lib.prg_debug_gn_stats(a["x"], a["slabs"], a["ns"], a["B"], a["C"], a["HW"], a["G"], a["dtype"], None),
          good, bad)
    assert ns.value == -5 and all(v == -7.0 for v in host["buf"])


def test_gn_coeff_rejects_bad_arguments(host):
    lib, p = _lib.load(), host["p"]
    row = C.c_int(2)
    neg, far = C.c_int(-1), C.c_int(9)
    plain = dict(slabs=p, ns=4, gamma=p, beta=p, ss_a=None, sa=0, na=0, ss_b=None, sb=0, nb=0, row=None, rs=0, A=p, Bc=p, B=2, HW=64, C=64, G=8)
    cond = dict(plain, ss_a=p, sa=0, na=5 * 152, row=C.byref(row), rs=152, ss_b=p, sb=152, nb=2 * 152)
    call = lambda a: lib.prg_debug_gn_coeff(a["slabs"], a["ns"], a["gamma"], a["beta"], a["ss_a"], a["sa"], a["na"], a["ss_b"], a["sb"], a["nb"],
                                            a["row"], a["rs"], a["A"], a["Bc"], a["B"], a["HW"], a["C"], a["G"], None)
    sweep(lib, "prg_debug_gn_coeff", call, plain,
          [dict(slabs=None), dict(gamma=None), dict(beta=None), dict(A=None), dict(Bc=None), dict(ns=0), dict(ns=1025), dict(B=0), dict(B=65536),
           dict(HW=0), dict(C=0), dict(C=1032, G=8), dict(G=0), dict(G=65, C=65), dict(G=7), dict(ss_b=p, sb=128, nb=256), dict(row=C.byref(row))])
    sweep(lib, "prg_debug_gn_coeff", call, cond,
          [dict(sa=-1), dict(rs=-1), dict(na=0), dict(na=2 * 152 + 127),          # row 2 of rows 152 wide: 128 floats from 304
           dict(row=C.byref(neg)), dict(row=C.byref(far)), dict(sa=500),          # image 1 leaves the array
           dict(sb=-1), dict(nb=0), dict(nb=152 + 127), dict(sb=200)])
    assert all(v == -7.0 for v in host["buf"])


def test_gn_fold_rejects_bad_arguments(host):
    lib, p = _lib.load(), host["p"]
    ent = (C.c_int64 * 8)(16, 64, 0, 64, 200, 128, 128, 256)
    ep = C.cast(ent, C.c_void_p).value
    row = C.c_int32(1)
    tables = dict(acc=p, p=p, q=p, coef_a=p, coef_b=p, B=2, C=64, HW=64, groups=8, output=_lib.GF_TABLES)
    apply_ = dict(acc=p, p=p, q=p, x=p, out=p, B=2, C=64, HW=64, groups=8, output=_lib.GF_APPLY)
    cond = dict(entries=ep, n_entries=2, flat=p, flat_floats=384, ss_a=p, ss_a_stride=0, ss_a_floats=3 * 456, row=C.cast(C.pointer(row), C.c_void_p).value,
                row_stride=456, ss_b=p, ss_b_stride=456, ss_b_floats=2 * 456, ss_total=456, pq=p, zero_out=p, zero_words=100, B=2, output=_lib.GF_NONE)
    cond_t = dict(cond, acc=p, coef_a=p, coef_b=p, C=128, HW=64, groups=8, use_entry=1, output=_lib.GF_TABLES)

    def call(a):
        s = _lib.GnFoldC(**a)
        return lib.prg_debug_gn_fold(C.byref(s), None)

    n = sweep(lib, "prg_debug_gn_fold", call, tables,
              [dict(acc=None), dict(p=None), dict(q=None), dict(coef_a=None), dict(coef_b=None), dict(B=0), dict(B=65536), dict(C=0), dict(C=8192),
               dict(groups=0), dict(groups=7), dict(HW=0), dict(output=3), dict(output=-1), dict(output=_lib.GF_NONE), dict(pq_per_image=2),
               dict(in_place=1), dict(in_place=2), dict(residual=p)])
    n += sweep(lib, "prg_debug_gn_fold", call, apply_,
               [dict(x=None), dict(out=None), dict(C=60, groups=4), dict(C=2048), dict(B=4096, HW=4096), dict(in_place=-1)])
    n += sweep(lib, "prg_debug_gn_fold", call, cond,
               [dict(p=p), dict(q=p), dict(pq_per_image=1), dict(n_entries=0), dict(n_entries=257), dict(ss_total=0), dict(flat=None), dict(flat_floats=0),
                dict(ss_a=None), dict(pq=None), dict(zero_out=None), dict(zero_words=-1), dict(zero_words=1 << 25),
                dict(ss_total=455),                                               # entry 1 ends at 456
                dict(flat_floats=383),                                            # entry 1's beta ends at 384
                dict(ss_a_floats=2 * 456 - 1), dict(ss_b_floats=2 * 456 - 1), dict(ss_a_stride=-1), dict(row_stride=-1), dict(ss_b_stride=-1)])
    n += sweep(lib, "prg_debug_gn_fold", call, cond_t, [dict(use_entry=2), dict(use_entry=-1), dict(use_entry=0), dict(C=64), dict(acc=None)])
    assert n == 50
    assert lib.prg_debug_gn_fold(None, None) == PRG_E_INVALID and b"prg_debug_gn_fold" in lib.prg_last_error()
    assert all(v == -7.0 for v in host["buf"])


def test_affine_silu_rejects_bad_arguments(host):
    lib, p = _lib.load(), host["p"]
    good = dict(x=p, A=p, Bc=p, res=None, out=p, B=2, C=24, HW=50, dtype=_lib.PRG_BF16, in_place=0)
    bad = [dict(x=None), dict(A=None), dict(Bc=None), dict(out=None), dict(dtype=_lib.PRG_MXFP8), dict(dtype=_lib.PRG_F16X3), dict(dtype=7),
           dict(in_place=2), dict(in_place=-1), dict(C=0), dict(C=-8), dict(C=12), dict(C=6, dtype=_lib.PRG_F32), dict(B=0), dict(HW=0),
           dict(B=1 << 12, HW=1 << 14)]
    sweep(lib, "prg_debug_affine_silu", lambda a: lib.prg_debug_affine_silu(a["x"], a["A"], a["Bc"], a["res"], a["out"], a["B"], a["C"], a["HW"],
                                                                            a["dtype"], a["in_place"], None), good, bad)
    assert all(v == -7.0 for v in host["buf"])


def test_linear_rejects_bad_arguments(host):
    lib, p = _lib.load(), host["p"]
    good = dict(x=p, ldx=34, xoff=0, W=p, ldw=34, woff=17, bias=None, y=p, ldy=49, ycol=24, R=65, I=17, O=9, ai=1, ao=0)
    bad = [dict(x=None), dict(W=None), dict(y=None), dict(R=0), dict(R=-1), dict(R=(1 << 20) + 1), dict(I=0), dict(I=1 << 17), dict(O=0), dict(O=1 << 17),
           dict(xoff=-1), dict(xoff=18), dict(ldx=16), dict(woff=-1), dict(woff=18), dict(ldw=33), dict(ycol=-1), dict(ycol=41), dict(ldy=32),
           dict(ldx=(1 << 20) + 1), dict(R=1 << 20, ldx=1 << 10), dict(ai=3), dict(ai=-1), dict(ao=3), dict(ao=-1)]
    sweep(lib, "prg_debug_linear", lambda a: lib.prg_debug_linear(a["x"], a["ldx"], a["xoff"], a["W"], a["ldw"], a["woff"], a["bias"], a["y"], a["ldy"],
                                                                  a["ycol"], a["R"], a["I"], a["O"], a["ai"], a["ao"], None), good, bad)
    assert all(v == -7.0 for v in host["buf"])


def test_sinusoidal_rejects_bad_arguments(host):
    lib, p = _lib.load(), host["p"]
    good = dict(t=p, freqs=p, out=p, R=4, dim=64, wide=1)
    bad = [dict(t=None), dict(freqs=None), dict(out=None), dict(R=0), dict(R=-3), dict(dim=2), dict(dim=0), dict(dim=65), dict(wide=2), dict(wide=-1),
           dict(R=1 << 20, dim=64)]
    sweep(lib, "prg_debug_sinusoidal", lambda a: lib.prg_debug_sinusoidal(a["t"], a["freqs"], a["out"], a["R"], a["dim"], a["wide"], None), good, bad)
    assert all(v == -7.0 for v in host["buf"])
