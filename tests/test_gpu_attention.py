"""The attention kernels alone, each against a float64 reference of the same operation on exactly the values it receives:
the generic, bf16-MFMA and split-f16 bottleneck cores and the linear core (prg_debug_attention_core), the channel LayerNorm
(prg_debug_layernorm) and the fused / split Residual(PreNorm(LinearAttention)) blocks (prg_debug_linear_attention_block).
Families, references, tolerances and their derivations: tests/test_attention_refs.py.  Every case prints its observed error
against its tolerance.

Observed on an MI355X, largest error / tolerance over all cases (the bf16 figures near 1 are the half ulp of the bf16 store, which is
the dominant term of those bounds and is reached by some element of every large output):
  generic    f32 0.04, bf16 0.94               mfma bf16 0.31 (0.0078 .. 0.0152 against 0.030 .. 0.050)
  split      f16x3 0.015 (9.2e-6 at N = 1024)  linear     f32 0.11, bf16 0.99
  layernorm  f32 0.26, bf16 1.00 (1.561e-2 against half an ulp of 1.5625e-2 plus 3e-6)
  fused bf16 blocks   max 2.0e-2 .. 4.5e-2, mean 1.7e-3 .. 2.7e-3: both within 1 % of the emulation's figures in every case
                      family E, 120 cases (every C, N, B, psum with static shifts and with measured maxima): max 2.0e-2 .. 3.1e-2,
                      mean / emulated mean 0.993 .. 1.003; static against measured differ by 7.8e-3 .. 3.1e-2 (one or two bf16
                      ulps of the output, 0.37 .. 1.56 of the emulation's maximum, bound 3)
  split f16x3 blocks  1.1e-6 .. 1.5e-6 against an emulated 1.0e-6 .. 1.5e-6 (bound 4.0e-6 .. 6.1e-6, cap 1.5e-4 .. 1.8e-4)
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pointreggpt_amd import _lib
from test_attention_refs import (BLOCK_N_BF16, BLOCK_N_SPLIT, DH, FULL_GENERIC_N, FULL_MFMA_N, FULL_SPLIT_N, HEADS, HID, LINEAR_N, LN_C_BF16,
                                 LN_C_F32, LN_M, STATIC_LIMIT, bf16, block_case, full_tol, layernorm_inputs, layernorm_tol, linear_tol,
                                 make_qkv, ref_full, ref_layernorm, ref_linear, static_bounds)

pytestmark = pytest.mark.gpu

DTYPE = {"f32": _lib.PRG_F32, "bf16": _lib.PRG_BF16, "f16x3": _lib.PRG_F16X3}
FAMILIES = ("F1", "F2", "F3", "F4_nan_v", "F4_nan_k", "F4_inf_v")
PRG_E_INVALID = -1


def run_core(qkv, dtype, linear, kernel):
    lib = _lib.load()
    B, _, N = qkv.shape
    d_qkv = qkv.float().contiguous().cuda()
    out = torch.full((B, HID, N), 7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.prg_debug_attention_core(_lib.ptr(d_qkv), _lib.ptr(out), B, N, DTYPE[dtype], linear, kernel, _lib.stream_ptr()),
               "prg_debug_attention_core")
    return out.cpu().double()


def check_core(label, out, ref, tol, images=None):
    """non-finite exactly where the reference is, the finite entries within the (image, head)'s tolerance"""
    assert torch.isfinite(out).all() or not torch.isfinite(ref).all(), label + ": non-finite output"
    if images is not None:
        out = out[images]
    B, _, N = ref.shape
    o, r = out.reshape(B, HEADS, DH, N), ref.reshape(B, HEADS, DH, N)
    fin = torch.isfinite(r)
    err = torch.where(fin, (o - r).abs(), torch.zeros_like(r))
    worst = (err / tol).amax()
    print(f"{label}: max |out - ref| = {float(err.max()):.3e}, tolerance {float(tol.min()):.3e} .. {float(tol.max()):.3e}, "
          f"largest error / tolerance = {float(worst):.3f}")
    assert torch.equal(torch.isnan(o), torch.isnan(r)), label + ": NaN pattern"
    assert torch.equal(torch.isposinf(o), torch.isposinf(r)) and torch.equal(torch.isneginf(o), torch.isneginf(r)), label + ": Inf pattern"
    assert bool((err <= tol).all()), f"{label}: error / tolerance = {float(worst):.3f}"


def core_case(family, B, N, dtype, linear):
    qkv = make_qkv(family, B, N, 1000 * B + N + (17 if linear else 0), linear=bool(linear))
    return bf16(qkv) if dtype == "bf16" else qkv


# generic kernel (full_attn_kernel<float> / <bf16_t>): KC = 128 chunk edges, the 256-query block edge, the clamp of the query index
@pytest.mark.parametrize("N", FULL_GENERIC_N)
@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_bottleneck_core_generic(dtype, N):
    for B in (1, 3):
        for fam in FAMILIES:
            qkv = core_case(fam, B, N, dtype, 0)
            tol, _ = full_tol(qkv, dtype)
            check_core(f"generic {dtype} {fam} B={B} N={N}", run_core(qkv, dtype, 0, 0), ref_full(qkv), tol)


def test_bottleneck_core_generic_is_what_f16x3_runs_without_its_kernel():
    qkv = core_case("F1", 3, 129, "f16x3", 0)
    out = run_core(qkv, "f16x3", 0, 0)
    check_core("generic f16x3 F1 B=3 N=129", out, ref_full(qkv), full_tol(qkv, "f32")[0])
    assert torch.equal(out, run_core(qkv, "f32", 0, 0))


def _matrix_pipe(label, dtype, variant, B, N, families):
    images = [0, 15, 31] if B == 32 else None
    for fam in families:
        qkv = core_case(fam, B, N, dtype, 0)
        sub = qkv if images is None else qkv[images]
        check_core(f"{label} {fam} B={B} N={N}", run_core(qkv, dtype, 0, 1), ref_full(sub), full_tol(sub, variant)[0], images)


# full_attn_mfma_kernel<2, 4, 8>, launch_attn_big<16, 2>, <32, 4> and (B = 32) <32, 2>
@pytest.mark.parametrize("B,N", [(3, n) for n in FULL_MFMA_N] + [(32, 1024)])
def test_bottleneck_core_bf16_mfma(B, N):
    _matrix_pipe("mfma bf16", "bf16", "mfma", B, N, FAMILIES if B == 3 else ("F1", "F2"))


# launch_fa<4, 1>, <8, 2>, <16, 4>, <32, 4> and (B = 32) <8, 1>, <32, 2>
@pytest.mark.parametrize("B,N", [(3, n) for n in FULL_SPLIT_N] + [(32, 256), (32, 1024)])
def test_bottleneck_core_f16x3_split(B, N):
    _matrix_pipe("split f16x3", "f16x3", "split", B, N, FAMILIES if B == 3 else ("F1", "F2"))


# slab = ceil(N / ceil(N / 512)), the 128-pixel slabs of the column maxima, more than one chunk of la_out
@pytest.mark.parametrize("N", LINEAR_N)
@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_linear_core(dtype, N):
    for B in (1, 3):
        for fam in FAMILIES:
            qkv = core_case(fam, B, N, dtype, 1)
            tol, _ = linear_tol(qkv, dtype)
            check_core(f"linear {dtype} {fam} B={B} N={N}", run_core(qkv, dtype, 1, 0), ref_linear(qkv), tol)


# ------------------------------------------------------------------------------------------------------------------------
def run_layernorm(x, g, res, dtype):
    lib = _lib.load()
    M, Cc = x.shape
    d_x = x.float().contiguous().cuda()
    d_r = None if res is None else res.float().contiguous().cuda()
    gh = np.ascontiguousarray(g.numpy(), dtype=np.float32)
    out = torch.full((M, Cc), 7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.prg_debug_layernorm(_lib.ptr(d_x), gh.ctypes.data_as(C.c_void_p), _lib.ptr(d_r), _lib.ptr(out), M, Cc, DTYPE[dtype],
                                       _lib.stream_ptr()), "prg_debug_layernorm")
    return out.cpu().double()


def check_layernorm(label, x, g, res, dtype):
    out, ref = run_layernorm(x, g, res, dtype), ref_layernorm(x, g, res)
    tol = layernorm_tol(x, g, ref, dtype, res)
    fin = torch.isfinite(ref)
    err = torch.where(fin, (out - ref).abs(), torch.zeros_like(ref))
    worst = torch.where(fin, err / tol, torch.zeros_like(ref)).amax()
    print(f"{label}: max |out - ref| = {float(err.max()):.3e}, largest error / tolerance = {float(worst):.3f}")
    assert torch.equal(torch.isnan(out), torch.isnan(ref)), label + ": NaN pattern"      # a NaN row stays NaN, and stays alone
    assert bool((err[fin] <= tol[fin]).all()), f"{label}: error / tolerance = {float(worst):.3f}"


# lane groups L = 1 .. 64, one or two vectors per lane (MAXV = 2: C = 512 in float32), a last block with idle lane groups
@pytest.mark.parametrize("dtype,Cc", [("f32", c) for c in LN_C_F32] + [("bf16", c) for c in LN_C_BF16])
def test_layernorm(dtype, Cc):
    for M in LN_M:
        for name, x, g, res in layernorm_inputs(M, Cc, dtype):
            check_layernorm(f"layernorm {dtype} C={Cc} M={M} {name}", x, g, res, dtype)


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_layernorm_grid_stride(dtype):
    """more rows than the capped grid of 16384 blocks x 4 rows covers in one pass"""
    M, Cc = 4 * 16384 + 5, 512
    g = torch.Generator().manual_seed(9)
    x = torch.randn((M, Cc), generator=g)
    check_layernorm(f"layernorm {dtype} C={Cc} M={M} normal", bf16(x) if dtype == "bf16" else x, 1 + 0.2 * torch.randn(Cc, generator=g), None, dtype)


# ------------------------------------------------------------------------------------------------------------------------
def run_block(W, x, dtype, shift_mode, psum):
    """(rc, out, used_static); out is None when the call was refused"""
    lib = _lib.load()
    B, Cc, N = x.shape
    host = {k: np.ascontiguousarray(v.numpy(), dtype=np.float32) for k, v in W.items()}
    hp = {k: v.ctypes.data_as(C.c_void_p) for k, v in host.items()}
    d_x = x.float().contiguous().cuda()
    out = torch.full((B, Cc, N), 7.0, dtype=torch.float32, device="cuda")
    used = C.c_int(-1)
    rc = lib.prg_debug_linear_attention_block(_lib.ptr(d_x), hp["norm_g"], hp["w_qkv"], hp["w_out"], hp["b_out"], hp["out_g"], _lib.ptr(out),
                                              B, Cc, N, DTYPE[dtype], shift_mode, psum, C.byref(used), _lib.stream_ptr())
    if rc == PRG_E_INVALID:
        return rc, None, used.value
    _lib.check(rc, "prg_debug_linear_attention_block")
    return rc, out.cpu().double(), used.value


def check_block(label, out, ref, emax, emean, kmax=3.0, kmean=2.0):
    assert torch.isfinite(out).all(), label + ": non-finite output"
    err = (out - ref).abs()
    print(f"{label}: max |out - ref| = {float(err.max()):.3e} (emulation {emax:.3e}), mean = {float(err.mean()):.3e} (emulation {emean:.3e})")
    assert float(err.max()) <= kmax * emax, f"{label}: max {float(err.max()):.3e} > {kmax} x {emax:.3e}"
    if kmean is not None:
        assert float(err.mean()) <= kmean * emean, f"{label}: mean {float(err.mean()):.3e} > {kmean} x {emean:.3e}"


# attn_fused.hip: less than one tile, a partial tile, one tile per block, a last slab of one tile, 25 tiles at three per block;
# the row sums of p on the matrix pipe or not; static shifts or measured maxima — the static shifts only where these realistic
# weights keep the bound, which is C = 64 alone (the hook must refuse them elsewhere): the static kernels of C = 128 and 256 run in
# the bound-edge test below, over the same grid.  The bound is measured, not derived (two softmaxes and
# a LayerNorm): 3 x the maximum and 2 x the mean error of the float64 emulation at the kernels' precision on the same inputs — the
# margins cover the accumulation order and the hardware exp2 / rsq, which the emulation does not model.
@pytest.mark.parametrize("N", BLOCK_N_BF16)
@pytest.mark.parametrize("Cc", (64, 128, 256))
def test_linear_attention_block_bf16(Cc, N):
    for B in (1, 3):
        W, x, ref, emax, emean = block_case(Cc, B, N, "R", "bf16")
        holds = float(static_bounds(W["w_qkv"], W["norm_g"]).max()) <= STATIC_LIMIT
        for shift_mode in (0, 1):
            for psum in (0, 1):
                rc, out, used = run_block(W, x, "bf16", shift_mode, psum)
                label = f"fused bf16 R C={Cc} B={B} N={N} shift_mode={shift_mode} psum={psum}"
                if shift_mode == 1 and not holds:
                    assert rc == PRG_E_INVALID and b"prg_debug_linear_attention_block" in _lib.load().prg_last_error(), label
                    continue
                assert rc == 0 and used == shift_mode, label
                check_block(label, out, ref, emax, emean)
        if "PRG_LA_KSHIFT" not in os.environ and "PRG_LA_PSUM" not in os.environ:
            rc, out, used = run_block(W, x, "bf16", -1, -1)          # the library's rule: static where the bound holds
            assert rc == 0 and used == int(holds)
            same = run_block(W, x, "bf16", int(holds), 1 if Cc >= 128 else 0)[1]
            assert torch.equal(out, same), f"fused bf16 R C={Cc} B={B} N={N}: the default is not the kernel it names"
        else:
            print(f"fused bf16 R C={Cc} B={B} N={N}: PRG_LA_KSHIFT / PRG_LA_PSUM is set, the library's own choice was NOT compared")


# exp2(k) with no shift near 2^+-56: every q / k row at a static bound of 56 log2 units (so the static shifts hold at EVERY width,
# which family R's weights allow only at C = 64: their bounds are 45, 58 and 82 against the limit of 57.7), the pixels aligned with a k
# row.  The whole grid of token counts, batch sizes and row-sum forms, with the static shifts and with the measured maxima:
# la_ctx_fused_kernel<C, false / true, true> and la_out_fused_kernel<C, true> run at every C on every tile and slab edge.
@pytest.mark.parametrize("N", BLOCK_N_BF16)
@pytest.mark.parametrize("Cc", (64, 128, 256))
def test_linear_attention_block_bf16_at_the_edge_of_the_static_bound(Cc, N):
    for B in (1, 3):
        W, x, ref, emax, emean = block_case(Cc, B, N, "E", "bf16")
        assert float(static_bounds(W["w_qkv"], W["norm_g"]).max()) <= STATIC_LIMIT
        for psum in (0, 1):
            outs = {}
            for shift_mode in (1, 0):
                rc, out, used = run_block(W, x, "bf16", shift_mode, psum)
                assert rc == 0 and used == shift_mode
                check_block(f"fused bf16 E C={Cc} B={B} N={N} shift_mode={shift_mode} psum={psum}", out, ref, emax, emean)
                outs[shift_mode] = out
            d = float((outs[1] - outs[0]).abs().max())
            print(f"fused bf16 E C={Cc} B={B} N={N} psum={psum}: max |static - measured| = {d:.3e} (emulation {emax:.3e})")
            assert d <= 3.0 * emax


# attn_split.hip: one tile, one tile per block, a last slab of one tile, 25 tiles.  4 x the emulation's maximum (the lo x lo term and
# the float32 accumulation are not modelled) and never more than the 2e-5 of the f16x3 taps.
@pytest.mark.parametrize("N", BLOCK_N_SPLIT)
@pytest.mark.parametrize("Cc", (64, 128))
def test_linear_attention_block_f16x3(Cc, N):
    W, x, ref, emax, _ = block_case(Cc, 3, N, "R", "f16x3")
    rc, out, used = run_block(W, x, "f16x3", -1, -1)
    assert rc == 0 and used == 0
    cap = 2e-5 * max(1.0, float(ref.abs().max()))
    check_block(f"split f16x3 R C={Cc} B=3 N={N} (cap {cap:.2e})", out, ref, min(4.0 * emax, cap), 0.0, kmax=1.0, kmean=None)
