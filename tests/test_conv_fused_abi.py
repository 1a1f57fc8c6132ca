"""The fused-conv test hook (prg_debug_conv_fused), checked without a GPU: header, binding, exported symbol, the argument struct's
layout against the header, and every PRG_E_INVALID case: all of them are rejected before the first device call, with the hook's
name in the message, so none needs a device."""
import ctypes as C
import os
import re

import pytest

from pointreggpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "prg_debug_conv_fused"
PRG_E_INVALID = -1
CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int64_t*": C.c_void_p, "int64_t*": C.c_void_p,
         "double*": C.c_void_p, "int32_t": C.c_int32}


def header():
    hdr = open(os.path.join(ROOT, "include", "prg.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def header_fields():
    """[(name, ctypes type)] of struct prg_conv_fused in declaration order"""
    m = re.search(r"typedef struct prg_conv_fused \{(.*?)\} prg_conv_fused;", header(), flags=re.S)
    assert m, "struct prg_conv_fused"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        t = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl)
        assert t and t.group(1) in CTYPE, decl
        fields += [(n.strip(), CTYPE[t.group(1)]) for n in t.group(2).split(",")]
    return fields


def test_hook_is_declared_bound_and_exported():
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", header())
    assert m, NAME
    assert [a.strip().split()[0] for a in m.group(1).split(",")] == ["prg_conv_fused*", "void*"]
    res, args = _lib.PROTOTYPES[NAME]
    assert res is C.c_int and args == [C.POINTER(_lib.ConvFusedC), C.c_void_p]
    assert hasattr(C.CDLL(str(_lib.LIB_PATH)), NAME)


def test_struct_layout_matches_the_header():
    fields = header_fields()
    assert [(n, t) for n, t in _lib.ConvFusedC._fields_] == fields
    # the C layout of the header's declaration: natural alignment, in order
    off = 0
    for name, t in fields:
        size = C.sizeof(t)
        off = (off + size - 1) // size * size
        assert getattr(_lib.ConvFusedC, name).offset == off, name
        off += size
    assert C.sizeof(_lib.ConvFusedC) == (off + 7) // 8 * 8 == 20 * 8 + 22 * 4
    # `storage` took the place of `reserved`: every earlier field keeps its offset, the out-fields and `slabs` follow it
    assert _lib.ConvFusedC.storage.offset == 19 * 8 + 15 * 4 and _lib.ConvFusedC.stats_pass.offset == 19 * 8 + 14 * 4
    assert [n for n, _ in fields[-8:]] == ["storage", "family", "th", "tw", "bm", "bn", "nslabs", "slabs"]
    hdr = header()
    for group, names in (("PRO", ("NONE", "TABLES", "FOLD")), ("RES", ("NONE", "ADD", "TABLES", "FOLD")), ("STATS", ("OFF", "SLABS", "ACC")),
                         ("STORE", ("BF16", "F16X3", "F32"))):
        for value, n in enumerate(names):
            assert re.search(rf"PRG_CF_{group}_{n} = {value}\b", hdr), (group, n)
            assert getattr(_lib, f"CF_{group}_{n}") == value
    assert re.search(r"PRG_CF_MAX_SLABS = 1024\b", hdr) and _lib.CF_MAX_SLABS == 1024
    # the family names of the binding follow the enum of conv_choose.h
    enum = re.search(r"enum ConvFamily \{(.*?)\};", open(os.path.join(ROOT, "pointreggpt_amd", "csrc", "conv_choose.h")).read(), flags=re.S)
    names = re.findall(r"^\s*kConv(\w+)", enum.group(1), flags=re.M)
    assert [re.sub(r"(?<!^)(?=[A-Z])", "_", n).lower().replace("w256_mx", "w256mx") for n in names] == list(_lib.CONV_FAMILIES), names


@pytest.fixture(scope="module")
def host():
    """Host buffers that stand in for device pointers: an invalid call must return before anything looks at them."""
    buf = (C.c_float * 4096)(*[-7.0] * 4096)
    return dict(p=C.cast(buf, C.c_void_p).value, buf=buf)


def call(lib, **kw):
    a = _lib.ConvFusedC(**kw)
    return lib.prg_debug_conv_fused(C.byref(a), None)


def test_rejects_bad_arguments_before_any_device_call(host):
    lib, p = _lib.load(), host["p"]
    plain = dict(x0=p, w=p, bias=p, out=p, B=2, C0=64, C1=0, Cout=64, H=16, W=32, K=3, groups=8)
    two = dict(plain, x1=p, C1=64)
    pro_t = dict(plain, prologue=_lib.CF_PRO_TABLES, pro_a=p, pro_b=p)
    pro_f = dict(plain, prologue=_lib.CF_PRO_FOLD, fold_acc=p, fold_p=p, fold_q=p)
    one = dict(two, K=1, residual=p, residual_mode=_lib.CF_RES_ADD)
    res_t = dict(one, residual_mode=_lib.CF_RES_TABLES, res_a=p, res_b=p)
    res_f = dict(one, residual_mode=_lib.CF_RES_FOLD, fold_acc=p, fold_p=p, fold_q=p)
    st = dict(two, stats=_lib.CF_STATS_SLABS, gamma=p, beta=p, sums=p, coef_a=p, coef_b=p)
    st_acc = dict(st, stats=_lib.CF_STATS_ACC, acc_raw=p)
    bad = [
        (plain, [dict(x0=None), dict(w=None), dict(out=None), dict(B=0), dict(B=-1), dict(B=65536), dict(H=0), dict(W=-4),
                 dict(B=4096, H=64, W=64), dict(C0=0), dict(C0=60), dict(C0=-64), dict(C1=-8), dict(Cout=0), dict(Cout=68),
                 dict(K=0), dict(K=2), dict(K=4), dict(groups=0), dict(groups=-8), dict(groups=7),
                 dict(groups=16),                                                    # cpg = 4: cpg % 8 != 0
                 dict(Cout=72, groups=8),                                            # cpg = 9
                 dict(x1=p), dict(C1=64),                                            # x1 / C1 mismatch, both ways
                 dict(prologue=3), dict(prologue=-1), dict(residual_mode=4), dict(residual_mode=-1), dict(stats=3), dict(stats=-1),
                 dict(in_place=1), dict(in_place=2), dict(residual=p),               # residual / in_place without a residual mode
                 dict(storage=3), dict(storage=-1), dict(storage=255)]),             # storage outside 0 .. 2
        (two, [dict(x1=None), dict(C1=0), dict(C1=12)]),
        (pro_t, [dict(x1=p, C1=64),                                                  # a prologue with C1 > 0
                 dict(H=12, W=12),                                                   # a prologue on a 12x12 image
                 dict(Cout=72, groups=9), dict(K=1), dict(pro_a=None), dict(pro_b=None)]),
        (pro_f, [dict(x1=p, C1=64), dict(H=12, W=12), dict(fold_acc=None),           # fold mode without fold_acc
                 dict(fold_p=None), dict(fold_q=None),
                 dict(C0=72, Cout=64, groups=8)]),                                   # the folded tensor's cpg = 9
        (one, [dict(K=3),                                                            # a residual with K = 3
               dict(residual=None), dict(in_place=2), dict(in_place=-1)]),
        (res_t, [dict(K=3), dict(res_a=None), dict(res_b=None)]),
        (res_f, [dict(K=3), dict(fold_acc=None), dict(fold_p=None), dict(fold_q=None)]),
        (st, [dict(K=1),                                                             # statistics with K = 1
              dict(gamma=None), dict(beta=None), dict(sums=None), dict(coef_a=None), dict(coef_b=None),
              dict(Cout=2048, groups=8), dict(Cout=1024, groups=128)]),
        (st_acc, [dict(K=1), dict(acc_raw=None)]),
    ]
    # float storage: no folds and no accumulators (and a shape without a float kernel with a prologue: C0 % 32 != 0)
    for store in (_lib.CF_STORE_F16X3, _lib.CF_STORE_F32):
        bad += [(pro_f, [dict(storage=store)]), (res_f, [dict(storage=store)]), (st_acc, [dict(storage=store)]),
                (dict(pro_t, storage=store), [dict(C0=72), dict(x1=p, C1=64), dict(H=12, W=12), dict(pro_a=None)]),
                (dict(st, storage=store), [dict(K=1), dict(sums=None)]),
                (dict(res_t, storage=store), [dict(K=3), dict(res_b=None)])]
    n = 0
    for good, changes in bad:
        for change in changes:
            rc = call(lib, **dict(good, **change))
            assert rc == PRG_E_INVALID and NAME.encode() in lib.prg_last_error(), (change, lib.prg_last_error())
            n += 1
    assert lib.prg_debug_conv_fused(None, None) == PRG_E_INVALID and NAME.encode() in lib.prg_last_error()
    assert n == sum(len(changes) for _, changes in bad)
    assert all(v == -7.0 for v in host["buf"])
