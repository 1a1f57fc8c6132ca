"""The step schedule of conv3x3_c64_kernel (pointreggpt_amd/csrc/c64_schedule.h), proved on the CPU for every step count before
a kernel built on it is launched: the kernel's two wave classes meet only at workgroup barriers, so a barrier count that differs
between them is a hang, and a buffer rewritten an epoch too early is silent corruption.

The event rows come from prg_cpu_c64_schedule (libprg_cpu.so), which walks the same helper functions the kernel uses.  An event's
EPOCH is the number of barriers its role has executed before it: events of the two roles are ordered only when their epochs
differ (the earlier epoch happens first); inside one role program order holds."""
import ctypes as C

import numpy as np
import pytest

from pointreggpt_amd import cpu

PRODUCER, CONSUMER = 0, 1
ISSUE, WRITE, READ, BARRIER = 0, 1, 2, 3


def _events(nsteps, depth, role):
    lib = cpu.load()
    n = C.c_int64(0)
    cpu.check(lib.prg_cpu_c64_schedule(nsteps, depth, role, None, 0, C.byref(n)), "prg_cpu_c64_schedule")
    ev = np.full((n.value, 6), -7, dtype=np.int32)
    cpu.check(lib.prg_cpu_c64_schedule(nsteps, depth, role, ev.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "prg_cpu_c64_schedule")
    assert n.value == len(ev) and bool((ev[:, 0] == role).all())
    out, epoch = [], 0
    for pos, (_, kind, halo, rset, buf, tile) in enumerate(ev.tolist()):
        out.append(dict(kind=kind, halo=halo, set=rset, buf=buf, tile=tile, epoch=epoch, pos=pos))
        if kind == BARRIER:
            epoch += 1
    return out, epoch


CASES = [(n, d) for d in (2, 3) for n in range(1, 41)]


@pytest.fixture(scope="module")
def schedules():
    return {(n, d): (_events(n, d, PRODUCER), _events(n, d, CONSUMER)) for n, d in CASES}


@pytest.mark.parametrize("nsteps,depth", CASES)
def test_both_roles_execute_the_same_number_of_barriers(schedules, nsteps, depth):
    (_, pb), (_, cb) = schedules[nsteps, depth]
    assert pb == cb
    padded = -(-nsteps // depth) * depth
    assert pb == padded + 2


@pytest.mark.parametrize("nsteps,depth", CASES)
def test_every_halo_is_written_before_the_barrier_its_reader_waits_on(schedules, nsteps, depth):
    (prod, _), (cons, _) = schedules[nsteps, depth]
    reads = [e for e in cons if e["kind"] == READ]
    assert [e["halo"] for e in reads] == list(range(nsteps))         # every tile once, in order
    for r in reads:
        w = [e for e in prod if e["kind"] == WRITE and e["halo"] == r["halo"]]
        assert len(w) == 1 and w[0]["buf"] == r["buf"] and w[0]["tile"] == r["tile"] == r["halo"]
        assert w[0]["epoch"] < r["epoch"]                            # a barrier lies between the write and the read


@pytest.mark.parametrize("nsteps,depth", CASES)
def test_no_lds_buffer_is_rewritten_before_its_last_readers_barrier(schedules, nsteps, depth):
    (prod, _), (cons, _) = schedules[nsteps, depth]
    reads = [e for e in cons if e["kind"] == READ]
    for w in (e for e in prod if e["kind"] == WRITE):
        assert w["buf"] in (0, 1)
        for r in reads:
            if r["buf"] != w["buf"] or r["halo"] == w["halo"]:
                continue
            # a read of ANOTHER halo in the same buffer is over (earlier epoch) or not begun and fed by a later write
            if r["halo"] < w["halo"]:
                assert r["epoch"] < w["epoch"], (w, r)
            else:
                assert r["epoch"] > w["epoch"], (w, r)


@pytest.mark.parametrize("nsteps,depth", CASES)
def test_no_register_set_is_reloaded_before_it_was_written_out(schedules, nsteps, depth):
    (prod, _), _ = schedules[nsteps, depth]
    holds = {}                                                       # register set -> halo whose loads it holds, not yet written
    issued_at = {}
    for e in prod:
        if e["kind"] == ISSUE:
            assert 0 <= e["set"] < depth
            assert e["set"] not in holds, (e, holds)                 # the set's previous halo has gone to LDS
            holds[e["set"]] = e["halo"]
            issued_at[e["halo"]] = e["epoch"]
        elif e["kind"] == WRITE:
            assert holds.get(e["set"]) == e["halo"], (e, holds)      # the set still holds the halo being written
            del holds[e["set"]]
            # the loads had depth - 1 whole steps to land (the halos the prologue issues first have fewer: it has no steps before it)
            if e["halo"] >= depth - 1:
                assert e["epoch"] - issued_at[e["halo"]] == depth - 1, e
            elif e["halo"] > 0:
                assert e["epoch"] - issued_at[e["halo"]] >= 1, e
    assert len(holds) == depth - 1                                   # what is left are clamped reloads nobody writes or reads


@pytest.mark.parametrize("nsteps,depth", CASES)
def test_padded_steps_are_never_read(schedules, nsteps, depth):
    (prod, _), (cons, cb) = schedules[nsteps, depth]
    assert all(e["halo"] < nsteps for e in cons if e["kind"] == READ)
    last_read_epoch = max(e["epoch"] for e in cons if e["kind"] == READ)
    for e in prod:
        if e["kind"] in (ISSUE, WRITE) and e["halo"] >= nsteps:
            assert e["tile"] == nsteps - 1                           # a clamped reload of the last tile: an address inside the tensor
        if e["kind"] == WRITE and e["halo"] >= nsteps and e["buf"] == (nsteps - 1) & 1:
            assert e["epoch"] > last_read_epoch                      # padding never lands under the last tile's reads
    assert sum(1 for e in cons if e["kind"] == BARRIER) == cb


def test_bad_arguments_are_refused():
    lib = cpu.load()
    n = C.c_int64(0)
    for nsteps, depth, role in ((0, 2, 0), (4, 4, 0), (4, 1, 1), (4, 3, 2)):
        assert lib.prg_cpu_c64_schedule(nsteps, depth, role, None, 0, C.byref(n)) != 0
    ev = np.zeros((2, 6), dtype=np.int32)
    assert lib.prg_cpu_c64_schedule(5, 3, 0, ev.ctypes.data_as(C.c_void_p), 2, C.byref(n)) != 0   # too small a buffer
