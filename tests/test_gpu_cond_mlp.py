"""The conditioning MLP kernels of blocks.hip alone through their test hooks (prg_debug_linear, prg_debug_sinusoidal) against the
float64 references of tests/test_norm_refs.py, whose docstring derives every tolerance used here: linear_kernel in the library's three
call forms over the sizes at which its row blocks, its 256-column LDS chunks and its two-outputs-per-wave rule change, and
sinusoidal_kernel<int32_t / int64_t>.  Every case prints its largest error / tolerance and asserts it <= 1; columns and rows the
launch must leave alone are compared bit for bit.

Observed on an MI355X, largest error / tolerance (all 12 cases pass; the module takes 2.2 s as a process of its own, nearly all of
it start-up: its calls add up to under 0.2 s):
  linear      GELU output 0.07 .. 0.42, plain 0.13 .. 0.98 (the bound there is the two float32 roundings and little else), the
              sampler's form (SiLU input, woff = e, null bias, a column offset into wider rows) 0.03 .. 0.44; every untouched column
              and guard row bit for bit.  1000 rows in one launch and in 16 launches of 64 rows: bit-identical in all three forms.
  sinusoidal  int32 0.12 .. 0.21, int64 0.12 .. 0.21 (K_SIN = 4 ulp allowed, under one ulp observed), t = 2^32 + 5 included.
No case failed at any point: these tests found no defect in the kernels.
"""
import pytest
import torch

from pointreggpt_amd import _lib
from test_norm_refs import ACT_GELU, ACT_NONE, ACT_SILU, LINEAR_SIZES, linear_input, linear_reference, ratio, sampler_form, sinus_input, sinus_reference

pytestmark = pytest.mark.gpu


def dev(t, dtype=torch.float32):
    return t.to(dtype).contiguous().cuda()


def run_linear(d, rows=None):
    """the launch on rows [rows[0], rows[1]) of x and y (all by default); y with a guard row either side"""
    lib = _lib.load()
    lo, hi = rows or (0, d["R"])
    R = hi - lo
    x, W = dev(d["x"][lo:hi]), dev(d["W"])
    b = dev(d["bias"]) if d["bias"] is not None else None
    y = torch.full((R + 2, d["ldy"]), -7.0, dtype=torch.float32, device="cuda")
    y[1:-1] = dev(d["y"][lo:hi])
    rc = lib.prg_debug_linear(_lib.ptr(x), d["ldx"], d["xoff"], _lib.ptr(W), d["ldw"], d["woff"], _lib.ptr(b), y[1].data_ptr(), d["ldy"], d["ycol"],
                              R, d["I"], d["O"], d["act_in"], d["act_out"], _lib.stream_ptr())
    _lib.check(rc, "prg_debug_linear")
    y = y.cpu()
    assert bool((y[0] == -7.0).all()) and bool((y[-1] == -7.0).all()), "guard rows were written"
    return y[1:-1]


def forms(seed, R, I, O):
    return {"gelu_out": linear_input(seed, R, I, O, act_out=ACT_GELU), "plain": linear_input(seed + 1, R, I, O, act_in=ACT_NONE),
            "sampler": sampler_form(seed + 2, R, I, O)}


@pytest.mark.parametrize("sizes", LINEAR_SIZES, ids=lambda s: f"R{s[0]} I{s[1]} O{s[2]}")
def test_linear_call_forms(sizes):
    R, I, O = sizes
    worst = {}
    for name, d in forms(100 + LINEAR_SIZES.index(sizes), R, I, O).items():
        ref, tol = linear_reference(d)
        if name == "sampler":
            assert d["bias"] is None and d["woff"] == I and d["ldw"] == 2 * I and d["ldy"] > O and d["ycol"] > 0 and d["act_in"] == ACT_SILU
            assert int((tol == 0).sum()) == R * (d["ldy"] - O)               # untouched columns: bit for bit
        worst[name] = ratio(run_linear(d), ref, tol)
    print(f"linear (R, I, O) = {sizes}: largest error / tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_linear_is_independent_of_the_launch_shape():
    # prg_sampler_create's 1000 rows in one launch (16 row blocks, the last one ragged) and in launches of 64 rows
    for name, d in forms(200, 1000, 64, 130).items():
        whole = run_linear(d)
        parts = torch.cat([run_linear(d, (lo, min(1000, lo + 64))) for lo in range(0, 1000, 64)])
        assert torch.equal(whole, parts), name
        ref, tol = linear_reference(d)
        q = ratio(whole, ref, tol)
        print(f"linear 1000 rows, {name}: one launch and 16 launches of 64 rows bit-identical; largest error / tolerance {q:.3g}")
        assert q <= 1.0


def run_sinusoidal(t, freqs, dim, wide):
    lib = _lib.load()
    R = len(t)
    dt, df = torch.from_numpy(t).cuda(), torch.from_numpy(freqs).cuda()
    out = torch.full((R + 2, dim), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.prg_debug_sinusoidal(_lib.ptr(dt), _lib.ptr(df), out[1].data_ptr(), R, dim, wide, _lib.stream_ptr()), "prg_debug_sinusoidal")
    out = out.cpu()
    assert bool((out[0] == -7.0).all()) and bool((out[-1] == -7.0).all()), "guard rows were written"
    return out[1:-1]


# (dim, R): R dim / 2 below, at and above one block of 256 threads
SINUS = [(4, 4), (4, 128), (4, 129), (6, 85), (6, 86), (64, 7), (64, 8), (64, 9), (130, 4)]


@pytest.mark.parametrize("wide", (0, 1), ids=("int32", "int64"))
def test_sinusoidal(wide):
    worst = {}
    for dim, R in SINUS:
        t, freqs = sinus_input(R, dim, wide)
        assert {0, 1, 999} <= set(t.tolist()) and (not wide or (t > 2 ** 32).any())
        ref, tol = sinus_reference(t, freqs)
        worst[f"dim{dim}_R{R}"] = ratio(run_sinusoidal(t, freqs, dim, wide), ref, tol)
    print(f"sinusoidal {'int64' if wide else 'int32'}: largest error / tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
