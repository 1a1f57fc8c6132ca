"""The fused ResnetBlock tail kernel alone (prg_debug_resblock_tail) against a float64 reference of the same formula,

    out[b, n, c] = SiLU(h[b, n, c] * A[b, c] + Bc[b, c]) + sum_k w_res[c, k] * cat[s0, s1][b, n, k] + b_res[c]
    head[b, n]   = sum_c head_w[c] * out[b, n, c] + head_b            (optionally through a sigmoid)

on inputs first rounded to bf16 (h, s0, s1, w_res: what the kernel reads; A, Bc, b_res, head_w, head_b stay float32).

Shapes.  The kernel walks T = 8 tiles of 64 pixels per block and keeps D = 2 tiles of reads in flight, so N covers: less than a
tile (4), one tile (64), a partial second tile (100), exactly the prefetch depth (64 D), the depth plus a partial tile (64 D + 4),
one full block (64 T), a second block of one tile (64 T + 64), and two blocks plus a block with an odd number of tiles whose last
one is partial (64 (2 T + 1) + 36).  B = 1 and 3; the three channel configurations the library instantiates; the bf16 h buffer
as the output buffer or not; the 1x1 head (Cout = 64 only) with and without its sigmoid.

Tolerance (derived, per element; u = h A + Bc, P = sum_k |w||x|, e = 2^-24 the float32 unit roundoff):
  float32 terms  t32 = |SiLU(u)| (|u| + 6) 2 e     v_exp_f32 and v_rcp_f32 at 1 ulp each, the two roundings around them, and the
                                                   rounding of the exponent's argument (|u| log2 e, relative e), which v_exp_f32
                                                   turns into a relative error of |u| ln 2 log2 e e = |u| e
                     + 1.1 |u| e                   the rounding of the fmaf through |SiLU'| <= 1.1
                     + CIN e P                     float32 accumulation of CIN exact bf16 x bf16 products
                     + 2 e (|SiLU(u)| + P + |b_res|)   the two float32 additions
  bf16 store     half an ulp of bf16 at the output: 2^(E - 8) for 2^E <= |v| < 2^(E + 1), taken at |ref| + t32 (between 2^-9 |v| and
                 2^-8 |v|; the upper end is reached just above a power of two)
  head           sum_c |head_w[c]| (one bf16 ulp of out[c] + t32[c]) + (Cout + 2) e (sum_c |head_w[c] out[c]| + |head_b|);
                 with the sigmoid, a quarter of that (|sigmoid'| <= 1/4) + 4 e (expf, the division, two roundings)
Every case prints its largest error / tolerance.

Observed on an MI355X, largest error / tolerance over the cases: tensor output 0.96 .. 1.00 (the half ulp of the bf16 store is the
dominant term and some element of every output comes within a float32 rounding of it), head output 0.05 .. 0.24.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from pointreggpt_amd import _lib

pytestmark = pytest.mark.gpu

T_TILES, DEPTH = 8, 2
N_CASES = (4, 64, 100, 64 * DEPTH, 64 * DEPTH + 4, 64 * T_TILES, 64 * T_TILES + 64, 64 * (2 * T_TILES + 1) + 36)
CONFIGS = ((64, 64, 64), (128, 64, 128), (128, 128, 128))
GUARD = 1024       # float32 guard elements on either side of `out`
EPS = 2.0 ** -24


def bf16(x):
    return x.to(torch.bfloat16).double()


def inputs(C0, C1, Cout, B, N, kind, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    d = dict(h=bf16(rn(B, N, Cout)), s0=bf16(rn(B, N, C0)), s1=bf16(rn(B, N, C1)),
             A=(1.0 + 0.3 * rn(B, Cout)).float(), Bc=(0.5 * rn(B, Cout)).float(),
             w=bf16(rn(Cout, C0 + C1) * (C0 + C1) ** -0.5), b=(0.2 * rn(Cout)).float(),
             hw=(rn(Cout) * Cout ** -0.5).float(), hb=(0.1 * rn(1)).float())
    if kind == "tails":            # |h A + Bc| up to ~100: exp2 overflows to +inf on one side and underflows on the other
        d["A"] = (25.0 * (1.0 + 0.3 * rn(B, Cout))).float()
        d["Bc"] = (10.0 * rn(B, Cout)).float()
    elif kind == "zero_sources":
        d["s0"].zero_()
        d["s1"].zero_()
    return d


def half_ulp_bf16(v):
    """2^(E - 8) for 2^E <= v < 2^(E + 1) (bf16: 8 significant bits); 0 stays 0"""
    _, ex = torch.frexp(v.clamp(min=2.0 ** -120))
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), ex - 9), torch.zeros_like(v))


def reference(d, head, sigmoid):
    """(ref, tol) in float64"""
    cin = d["w"].shape[1]
    x = torch.cat([d["s0"], d["s1"]], dim=2)
    u = d["h"] * d["A"].double()[:, None, :] + d["Bc"].double()[:, None, :]
    silu = u * torch.sigmoid(u)
    acc = torch.einsum("bnk,ck->bnc", x, d["w"])
    P = torch.einsum("bnk,ck->bnc", x.abs(), d["w"].abs())
    bres = d["b"].double()
    ref = silu + acc + bres
    t32 = silu.abs() * (u.abs() + 6.0) * 2 * EPS + 1.1 * u.abs() * EPS + cin * EPS * P + 2 * EPS * (silu.abs() + P + bres.abs())
    hu = half_ulp_bf16(ref.abs() + t32)
    if not head:
        return ref, t32 + hu
    hw, hb = d["hw"].double(), d["hb"].double()
    y = ref @ hw + hb
    ty = (hw.abs() * (2 * hu + t32)).sum(dim=2) + (hw.numel() + 2) * EPS * ((ref * hw).abs().sum(dim=2) + hb.abs())
    if sigmoid:
        return torch.sigmoid(y), 0.25 * ty + 4 * EPS
    return y, ty


def run(d, head, sigmoid, in_place):
    lib = _lib.load()
    B, N, Cout = d["h"].shape
    C0, C1 = d["s0"].shape[2], d["s1"].shape[2]
    dev = {k: d[k].float().contiguous().cuda() for k in ("h", "s0", "s1", "A", "Bc")}
    host = {k: np.ascontiguousarray(d[k].float().numpy(), dtype=np.float32) for k in ("w", "b", "hw", "hb")}
    hp = {k: v.ctypes.data_as(C.c_void_p) for k, v in host.items()}
    n_out = B * N * (1 if head else Cout)
    big = torch.full((GUARD + n_out + GUARD,), 7.0, dtype=torch.float32, device="cuda")
    out = big[GUARD:GUARD + n_out]
    rc = lib.prg_debug_resblock_tail(_lib.ptr(dev["h"]), _lib.ptr(dev["s0"]), _lib.ptr(dev["s1"]), _lib.ptr(dev["A"]), _lib.ptr(dev["Bc"]),
                                     hp["w"], hp["b"], hp["hw"] if head else None, hp["hb"] if head else None, _lib.ptr(out), B, N, C0, C1,
                                     Cout, int(sigmoid), int(in_place), _lib.stream_ptr())
    _lib.check(rc, "prg_debug_resblock_tail")
    big = big.cpu()
    assert bool((big[:GUARD] == 7.0).all()) and bool((big[GUARD + n_out:] == 7.0).all()), "guard rows were written"
    return big[GUARD:GUARD + n_out].double().reshape((B, N) if head else (B, N, Cout))


def check(label, d, head=False, sigmoid=False, in_place=0):
    ref, tol = reference(d, head, sigmoid)
    out = run(d, head, sigmoid, in_place)
    assert torch.isfinite(out).all(), label + ": non-finite output"
    err = (out - ref).abs()
    worst = float((err / tol).amax())
    print(f"{label}: max |out - ref| = {float(err.max()):.3e}, largest error / tolerance = {worst:.3f}")
    assert bool((err <= tol).all()), f"{label}: error / tolerance = {worst:.3f}"
    return out


@pytest.mark.parametrize("N", N_CASES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "x".join(map(str, c)))
def test_tail_against_float64(cfg, N):
    C0, C1, Cout = cfg
    for B in (1, 3):
        d = inputs(C0, C1, Cout, B, N, "normal", 1000 * Cout + 10 * N + B + C0)
        outs = [check(f"tail {C0}+{C1}->{Cout} B={B} N={N} in_place={ip}", d, in_place=ip) for ip in (0, 1)]
        assert torch.equal(outs[0], outs[1]), "the in-place launch differs from the out-of-place one"


@pytest.mark.parametrize("N", N_CASES)
def test_tail_with_head_against_float64(N):
    for B in (1, 3):
        d = inputs(64, 64, 64, B, N, "normal", 77 * N + B)
        for sigmoid in (False, True):
            for ip in (0, 1):
                check(f"tail+head 64+64->64 B={B} N={N} sigmoid={int(sigmoid)} in_place={ip}", d, head=True, sigmoid=sigmoid, in_place=ip)


@pytest.mark.parametrize("kind", ("tails", "zero_sources"))
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "x".join(map(str, c)))
def test_tail_special_inputs(cfg, kind):
    C0, C1, Cout = cfg
    N = 64 * (2 * T_TILES + 1) + 36
    d = inputs(C0, C1, Cout, 3, N, kind, 5 + Cout + C0)
    if kind == "tails":
        u = d["h"] * d["A"].double()[:, None, :] + d["Bc"].double()[:, None, :]
        assert float(u.max()) > 88.0 and float(u.min()) < -88.0        # past expf's float32 range on both sides
    check(f"tail {C0}+{C1}->{Cout} {kind} N={N}", d, in_place=1)
    if Cout == 64:
        check(f"tail+head {kind} N={N}", d, head=True, sigmoid=True, in_place=1)
