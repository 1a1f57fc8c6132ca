"""The objective interface, checked without a GPU: the headers, the two bindings, the exported symbols, the unchanged prg_step, and
the PRG_E_INVALID cases of prg_debug_sampler_step_objective that are refused before any device call."""
import ctypes as C
import os
import re

from pointreggpt_amd import _lib, cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET, HOOK, TWIN = "prg_sampler_set_objective", "prg_debug_sampler_step_objective", "prg_cpu_sampler_run_objective"
P, I, F, L = C.c_void_p, C.c_int, C.c_float, C.c_int64


def declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return hdr, set(re.findall(r"\b(prg_[a-z0-9_]+)\s*\(", hdr))


def params(hdr, name):
    """The parameter list of `name`'s declaration as (type, name) pairs."""
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        out.append((p[:len(p) - len(p.split("*")[-1].split()[-1])].strip(), p.split("*")[-1].split()[-1]))
    return out


def ctype_of(decl):
    if decl.endswith("*"):
        return P
    return {"int": I, "float": F, "int64_t": L}[decl]


def test_prg_h_declares_binds_and_exports_the_two_entries():
    hdr, names = declared("prg.h")
    lib = C.CDLL(str(_lib.LIB_PATH))
    for name in (SET, HOOK):
        assert name in names and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert names == set(_lib.PROTOTYPES)
    res, args = _lib.PROTOTYPES[SET]
    assert res is C.c_int and args == [P, I, P, P, I]
    assert [n for _t, n in params(hdr, SET)] == ["h", "objective", "p", "q", "n"]
    assert [ctype_of(t) for t, _n in params(hdr, SET)] == args
    res, args = _lib.PROTOTYPES[HOOK]
    assert res is C.c_int and args[:15] == [P, P, P, P, P, I, F, F, F, P, I, I, I, C.POINTER(C.c_float), P] and len(args) == 15
    assert [n for _t, n in params(hdr, HOOK)] == ["x", "u", "img_cond", "seeds", "step", "objective", "p", "q", "keep_p", "keep_u", "B",
                                                 "HW", "reps", "avg_us", "stream"]
    assert [ctype_of(t) for t, _n in params(hdr, HOOK)] == [P, P, P, P, P, I, F, F, F, P, I, I, I, P, P]
    # the hook is the keep hook's argument list with (objective, p, q) put in after the row
    keep = _lib.PROTOTYPES["prg_debug_sampler_step_keep"][1]
    assert args[:5] == keep[:5] and args[8:] == keep[5:]


def test_prg_cpu_h_declares_binds_and_exports_the_twin():
    hdr, names = declared("prg_cpu.h")
    lib = C.CDLL(str(cpu.LIB_PATH))
    assert TWIN in names and TWIN in cpu.PROTOTYPES and hasattr(lib, TWIN)
    assert names == set(cpu.PROTOTYPES)
    res, args = cpu.PROTOTYPES[TWIN]
    keep = cpu.PROTOTYPES["prg_cpu_sampler_run_keep"][1]
    assert res is C.c_int and args == keep[:11] + [I, P, P] + keep[11:]          # run_keep's arguments plus objective, p, q
    got = params(hdr, TWIN)
    assert [n for _t, n in got][11:14] == ["objective", "p", "q"]
    assert [P if a is not I and a is not L else a for a in args] == [ctype_of(t) for t, _n in got]
    assert [n for _t, n in got][:11] + [n for _t, n in got][14:] == [n for _t, n in params(hdr, "prg_cpu_sampler_run_keep")]


def test_prg_step_and_the_abi_version_are_unchanged():
    assert [(n, t) for n, t in _lib.StepC._fields_] == [("t", C.c_int32), ("clip_pred", C.c_int32), ("c_x0", F), ("c_x", F), ("c_eps", F),
                                                        ("sigma", F), ("sqrt_recip", F), ("sqrt_recipm1", F)]
    assert C.sizeof(_lib.StepC) == 32
    hdr, _names = declared("prg.h")
    m = re.search(r"typedef struct prg_step \{(.*?)\} prg_step;", hdr, flags=re.S)
    fields = [" ".join(s.split()) for s in m.group(1).split(";") if s.strip()]
    assert fields == ["int32_t t", "int32_t clip_pred", "float c_x0, c_x, c_eps, sigma", "float sqrt_recip, sqrt_recipm1"]
    assert _lib.load().prg_abi_version() == 1
    for name in ("prg_sampler_create", "prg_sampler_run", "prg_sampler_set_keep", "prg_debug_sampler_step", "prg_debug_sampler_step_keep"):
        assert name in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["prg_sampler_run"][1] == [P, P, P, P, L, P, P, P]
    assert _lib.PROTOTYPES["prg_sampler_create"][1] == [P, C.POINTER(_lib.StepC), I, I, I, C.POINTER(P)]


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    step = _lib.StepC(0, 1, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0)
    buf = (C.c_float * 8)()
    a = C.cast(buf, P)
    for objective in (-1, 3, 99):
        assert lib.prg_debug_sampler_step_objective(a, a, None, a, C.byref(step), objective, 1.0, 1.0, -1.0, None, 1, 4, 1, None, None) == -1
        assert b"objective" in lib.prg_last_error()
    assert lib.prg_debug_sampler_step_objective(a, a, None, a, C.byref(step), 1, 1.0, 1.0, -1.0, None, 1, 6, 1, None, None) == -1   # HW % 4
    assert lib.prg_sampler_set_objective(None, 1, a, a, 1) == -1 and b"prg_sampler_set_objective" in lib.prg_last_error()
    assert bytes(buf) == bytes(32)
