"""Float64 references, input families and derived tolerances for the GroupNorm passes and the conditioning kernels of blocks.hip, each
run alone through its test hook (prg_debug_gn_stats, prg_debug_gn_coeff, prg_debug_gn_fold, prg_debug_affine_silu, prg_debug_linear,
prg_debug_sinusoidal), and their self-checks on the CPU.  tests/test_gpu_norm.py and tests/test_gpu_cond_mlp.py import this module.

Every operand is first rounded to its storage type (float32, or bf16 for the activations of the bf16 kernels), so the reference works on
the very numbers the kernel reads.  e = 2^-24 (half a float32 ulp, relative), d = 2^-53.  The library is built with -ffp-contract=off:
a product and a sum round separately unless the code says fmaf.  No tolerance is fitted to an observed error.

  gn_stats    slab k of image b covers pixels [k slab, min(HW, (k + 1) slab)), (nsplit, slab) from launch_gn_stats' formula.
              bf16: float32 accumulation, chain length depth = stat_depth("gn_stats", ...) (a thread's pixels, the psub sub-lanes, the
              group's channels): tol S = depth e sum |v|, tol Q = sum e v^2 (the rounded square) + depth e sum v^2.
              float: float64 accumulation and one rounding to float32 per slab: tol S = e |S| + depth d sum |v|, Q alike.
  gn_coeff    S, Q: float64 sums over the slabs (nsplit d sum |slab|); mean = S / n, var = max(Q / n - mean^2, 0) in float64: d var = 4 d
              (Q / n + mean^2) + the sums' share, so with |mean| / std = 2^8 (mean^2 / var = 2^16) var keeps 2^-34 of relative error:
              resolvable.  rstd = (var + 1e-5)^-1/2 and mean round once each to float32 (e each); a = rstd gamma (e |a|); b = beta -
              mean a (e |mean a| + e |b|).  Conditioning: s0 = ss_a + ss_b and s1 likewise round once each when ss_b is given (e |s0|,
              e |s1|), sc = s0 + 1 (e |sc|), a' = a sc (e |a'|), b' = fmaf(b, sc, s1) (e |b'|); the earlier errors go through the
              products: da' = da |sc| + |a| dsc + e |a'|, db' = db |sc| + |b| dsc + ds1 + e |b'|.
  cond_fold   P = gamma sc (|gamma| dsc + e |P|), Q = fmaf(beta, sc, s1) (|beta| dsc + ds1 + e |Q|); every other float of pq and every
              word of the accumulator array past zero_words is compared bit for bit.
  gn_fold     fold_coefficients of tests/test_conv_fused_refs.py (the dA / dB terms of gn_fold_stats_raw), with P, Q per image when
              pq_stride != 0; the pass is activation() of that module (silu_err for v_exp_f32 / v_rcp_f32), + e (|s| + |r|) for the
              residual's addition + half a bf16 ulp for the store.
  affine_silu bf16: the same with dA = dB = 0.  float: u = fmaf(x, A, B) (du = e |u|), y = u / (1 + expf(-u)): with E = exp(-u),
              |y| (K_EXP 2 e E / (1 + E) + e + e) + 1.1 du (expf, the sum's rounding, the division's; |SiLU'| <= 1.1), + e |y + r| for
              the residual.  u = -Inf gives NaN in both forms (-Inf / Inf, and -Inf * rcp(Inf) = -Inf * 0), as the float64 formula
              u sigmoid(u) = -Inf * 0 does.
  linear      the sum over i runs in float64 in index order on exact products (24 x 24 bits): I d sum |x w|; one rounding to float32
              (e |acc|), the float32 bias add (e |acc + bias|), the output activation: SiLU as above, GELU 0.5 v (1 + erff(v c)):
              |0.5 v| (1.13 e |v c| + K_ERF 2 e |erf| + e |1 + erf|) + e |g| + 1.13 dv  (|erf'| <= 2 / sqrt(pi) < 1.13, |GELU'| < 1.13).
              The input activation is float32: sum_i |W_oi| d(act_in(x_i)) with the same per-element bounds at dv = 0.
  sinusoidal  a = float32(t) freqs[i] is one IEEE float32 product, formed identically here; sin / cos of that a in float64;
              tolerance K_SIN ulps of a value in [1/2, 1): K_SIN 2^-24.

The ulp bounds of expf, erff, sinf, cosf: the ROCm installation these tests were written against carries no accuracy table (nothing
under share/doc, no statement in the HIP headers, the device library only as bitcode), so K_EXP = 3, K_ERF = 16, K_SIN = 4 are the
bounds of the OpenCL C specification (single precision: exp <= 3 ulp, erf <= 16 ulp, sin / cos <= 4 ulp), which the device library's
functions are written to conform to.

Self-checks: each mistake below is applied to the reference on the inputs the GPU tests use and measured in units of the tolerance
(largest error / tolerance; inf = a value that must match bit for bit did not, or NaN).  Recorded values:
  one slab left out: gn_stats 6.3e+04 .. 4.1e+05 (bf16), 1.7e+07 (float); gn_coeff, one of 257, 1.8e+05
  the last short slab read at full length (it runs into the next image): 44 (bf16, C = 8, HW = 5000: one pixel of 1667 too many)
      .. 4.8e+04 (bf16), 2.9e+05 .. 1.6e+07 (float); every other slab unchanged
  ss_b ignored 1.4e+07; row 0 used instead of *row 2.7e+07 (shared rows), 4.8e+07 (per-image rows); ss_a_stride taken as 0 4.3e+07,
      6.5e+07 with a row (image 0 cannot tell: 0); the + 1 on the scale forgotten 7.6e+07; the shift added before the scale 1.2e+07
  variance not clamped 4.3e+05 (the constant image, whose float32 slabs give Q / n < mean^2)
  eps outside the square root 42 (ordinary statistics, std in [0.5, 1.5]), 2.6e+09 (the constant image)
  group index c % G instead of c / cpg 4.6e+07 (C = 64, G = 8), 8.7e+07 (C = 1024, G = 64)
  the last 64 words not cleared: 64 wrong words at each zero_words (every word is compared: inf)
  woff ignored 8.1e+06; bias added on the null-bias call 2.8e+06; column O - 1 stored twice, into column O: inf (an untouched column
      changed); the I tail beyond 256 dropped 2.3e+07; cos and sin halves swapped 4.3e+06 .. 5.9e+06; only 32 bits of an int64 t read: > 1
A float32 evaluation of each formula on the CPU (test_*_passes, test_coeff_edges, test_apply_reference_*) stays inside the tolerances.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_conv_fused_refs import EPS, activation, fold_coefficients, fold_inputs, half_ulp_bf16, silu, stat_depth

D53 = 2.0 ** -53
K_EXP, K_ERF, K_SIN = 3, 16, 4
VEC = {"f32": 4, "bf16": 8}
PATTERN = 0x5A5A5A5A5A5A5A5A                      # what the hook fills the accumulator array with
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2


def store(x, dtype):
    """x rounded to the storage type, as float64"""
    return x.to(torch.bfloat16).double() if dtype == "bf16" else x.float().double()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ratio(got, ref, tol):
    """largest |got - ref| / tol; where tol = 0 or ref is NaN the values must agree exactly (inf otherwise); a non-finite `got` where
    the reference is finite counts as inf"""
    got, ref, tol = got.double(), ref.double(), tol.double().expand_as(ref)
    q = (got - ref).abs() / tol.clamp(min=1e-300)
    inf = torch.full_like(q, float("inf"))
    q = torch.where(torch.isfinite(got), q, inf)
    q = torch.where(got == ref, torch.zeros_like(q), q)
    q = torch.where((tol == 0) & (got != ref), inf, q)
    q = torch.where(torch.isnan(ref), torch.where(torch.isnan(got), torch.zeros_like(q), inf), q)
    return float(q.max()) if q.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# gn_stats
# ------------------------------------------------------------------------------------------------------------------------------
def stats_split(HW, C, vec):
    """(nsplit, slab, psub) of launch_gn_stats"""
    psub = 256 // (C // vec)
    ns = max(1, min(1024, -(-HW // (psub * 8))))
    slab = -(-HW // ns)
    return -(-HW // slab), slab, psub


def stats_input(seed, B, C, HW, dtype):
    g = gen(seed)
    amp = 0.5 + 1.5 * torch.rand(B, 1, 1, generator=g)
    off = amp * (torch.rand(B, 1, 1, generator=g) - 0.5)
    scale = 0.75 + 0.5 * torch.rand(1, C, 1, generator=g)
    return store((torch.randn(B, C, HW, generator=g) * amp + off) * scale, dtype)


def stats_reference(x, G, dtype, fault=None):
    """x (B, C, HW) float64 of storage values -> nsplit, sums (B, nsplit, G, 2), tol.  fault "full_last_slab": the last slab reads
    `slab` pixels, running into the next image (zeros behind the last one); "drop_slab": slab nsplit / 2 comes back as zeros"""
    B, C, HW = x.shape
    vec, cpg = VEC[dtype], C // G
    ns, slab, psub = stats_split(HW, C, vec)
    pad = ns * slab - HW
    xp = F.pad(x, (0, pad))
    if fault == "full_last_slab" and pad:
        xp[:, :, HW:] = torch.cat([x[1:], torch.zeros_like(x[:1])])[:, :, :pad]
    v = xp.reshape(B, G, cpg, ns, slab)
    red = lambda t: t.sum(dim=(2, 4)).permute(0, 2, 1)
    S, Q, Sa = red(v), red(v * v), red(v.abs())
    depth = -(-slab // psub) + psub + cpg
    if dtype == "bf16":
        assert depth == stat_depth("gn_stats", cpg, HW, C)
        tS, tQ = depth * EPS * Sa, EPS * Q + depth * EPS * Q
    else:
        tS, tQ = EPS * S.abs() + depth * D53 * Sa, EPS * Q + depth * D53 * Q
    sums = torch.stack([S, Q], dim=3)
    if fault == "drop_slab":
        sums[:, ns // 2] = 0.0
    return ns, sums, torch.stack([tS, tQ], dim=3)


# (name, dtype, B, C, HW, G): C / vec = 1 (psub 256), 256 (psub 1) and 16 or 8; HW < psub, a short last slab, one slab, the slab cap
STATS_CASES = [
    ("psub 256, HW < psub", "bf16", 2, 8, 4, 1),
    ("psub 256, short last slab", "bf16", 2, 8, 5000, 8),
    ("psub 256, HW < psub", "f32", 2, 4, 4, 1),
    ("psub 128, short last slab", "f32", 2, 8, 3001, 8),
    ("psub 1, one slab", "bf16", 2, 2048, 8, 64),
    ("psub 1, short last slab", "bf16", 2, 2048, 75, 8),
    ("psub 1, one slab", "f32", 2, 1024, 7, 64),
    ("psub 1, short last slab", "f32", 2, 1024, 75, 1),
    ("middle width, one slab", "bf16", 3, 64, 250, 8),
    ("middle width, short last slab", "bf16", 3, 64, 1093, 64),
    ("middle width, one slab", "f32", 3, 64, 120, 1),
    ("middle width, short last slab", "f32", 3, 64, 1093, 8),
    ("psub 1, the slab cap", "bf16", 1, 2048, 8200, 8),
    ("psub 1, the slab cap", "f32", 1, 1024, 8200, 64),
]


# ------------------------------------------------------------------------------------------------------------------------------
# gn_coeff
# ------------------------------------------------------------------------------------------------------------------------------
def coeff_input(seed, B, C, G, HW, ns, form="none", edge=None):
    """slabs (B, ns, G, 2) float32 of plausible statistics and one of the conditioning forms:
    "none"; "a_img": ss_a (B, 2C) per image; "sampler0" / "sampler_last": ss_a (T, W) shared by the batch (stride 0), row 0 or T - 1,
    ss_b (B, W) per image, both read at column offset 8 of rows W = 2C + 24 wide; "a_img_row": ss_a (B, T, 2C) per image with row.
    edge "constant": a constant image whose float32 slabs give Q / n < mean^2; "large_mean": |mean| / std = 2^8."""
    g = gen(seed)
    n = HW * (C // G)
    mean = 0.3 * torch.randn(B, 1, G, generator=g).double()
    std = 0.5 + torch.rand(B, 1, G, generator=g).double()
    if edge == "large_mean":
        mean, std = torch.full_like(mean, 128.0) * torch.where(torch.arange(G) % 2 == 0, 1.0, -1.0), torch.full_like(std, 0.5)
    nk = n / ns
    mk = mean + 0.2 * std * torch.randn(B, ns, G, generator=g).double()
    qk = mk * mk + std * std * (0.5 + torch.rand(B, ns, G, generator=g).double())
    slabs = torch.stack([mk * nk, qk * nk], dim=3).float()
    if edge == "constant":
        s = torch.full((B, ns, G), 3.0 * nk, dtype=torch.float32)
        q = torch.nextafter(torch.full((B, ns, G), 9.0 * nk, dtype=torch.float32), torch.tensor(0.0))
        slabs = torch.stack([s, q], dim=3)
    d = dict(B=B, C=C, G=G, HW=HW, ns=ns, slabs=slabs, form=form, edge=edge,
             gamma=(1.0 + 0.3 * torch.randn(C, generator=g)).float(), beta=(0.5 * torch.randn(C, generator=g)).float(),
             ss_a=None, ss_b=None, row=None, ss_a_stride=0, ss_b_stride=0, row_stride=0, ss_off=0)
    rn = lambda *s: (0.4 * torch.randn(*s, generator=g)).float()
    T, W = 5, 2 * C + 24
    if form == "a_img":
        d.update(ss_a=rn(B, 2 * C), ss_a_stride=2 * C)
    elif form in ("sampler0", "sampler_last"):
        d.update(ss_a=rn(T, W), ss_a_stride=0, row=0 if form == "sampler0" else T - 1, row_stride=W, ss_b=rn(B, W), ss_b_stride=W, ss_off=8)
    elif form == "a_img_row":
        d.update(ss_a=rn(B, T, 2 * C), ss_a_stride=T * 2 * C, row=3, row_stride=2 * C)
    return d


def cond_rows(d, width, off, fault=None):
    """(s0 + s1 rows (B, width) float64, their rounding error bound): GnApply's addressing at column `off`"""
    B = d["B"]
    a = d["ss_a"].reshape(-1).double()
    row = d["row"] if d["row"] is not None and fault != "row0" else 0
    stride = 0 if fault == "stride0" else d["ss_a_stride"]
    base = torch.arange(B) * stride + row * d["row_stride"] + off
    idx = base[:, None] + torch.arange(width)[None]
    s = a[idx]
    err = torch.zeros_like(s)
    if d["ss_b"] is not None and fault != "no_ss_b":
        bidx = (torch.arange(B) * d["ss_b_stride"] + off)[:, None] + torch.arange(width)[None]
        s = s + d["ss_b"].reshape(-1).double()[bidx]
        err = EPS * s.abs()
    return s, err


def coeff_reference(d, fault=None):
    """A, Bc, tol A, tol Bc (B, C) float64 of gn_coeff_kernel.  fault: "drop_slab", "no_ss_b", "row0", "stride0", "no_plus1",
    "shift_first", "no_clamp", "eps_outside", "c_mod_G"."""
    B, C, G, HW, ns = d["B"], d["C"], d["G"], d["HW"], d["ns"]
    cpg, n = C // G, float(HW * (C // G))
    sl = d["slabs"].double()
    if fault == "drop_slab":
        sl = torch.cat([sl[:, :ns // 2], sl[:, ns // 2 + 1:]], dim=1)
    S, Q = sl[..., 0].sum(dim=1), sl[..., 1].sum(dim=1)
    dS, dQ = ns * D53 * sl[..., 0].abs().sum(dim=1), ns * D53 * sl[..., 1].abs().sum(dim=1)
    mean = S / n
    var = Q / n - mean * mean
    if fault != "no_clamp":
        var = var.clamp(min=0.0)
    dmean = dS / n + D53 * mean.abs()
    dvar = 4 * D53 * (Q / n + mean * mean) + dQ / n + 2 * mean.abs() * dmean
    rstd = 1.0 / (var.sqrt() + 1e-5) if fault == "eps_outside" else (var + 1e-5) ** -0.5
    drstd = ((var - dvar).clamp(min=0.0) + 1e-5) ** -0.5 - rstd + 8 * D53 * rstd + EPS * rstd
    dmean = dmean + EPS * mean.abs()
    if fault == "c_mod_G":
        ch = lambda t: t[:, torch.arange(C) % G]
    else:
        ch = lambda t: t.repeat_interleave(cpg, dim=1)
    gam, bet = d["gamma"].double()[None], d["beta"].double()[None]
    a = ch(rstd) * gam
    b = bet - ch(mean) * a
    da = gam.abs() * ch(drstd) + EPS * a.abs()
    db = a.abs() * ch(dmean) + ch(mean.abs()) * da + EPS * (ch(mean) * a).abs() + EPS * b.abs()
    if d["ss_a"] is not None:
        s, ds = cond_rows(d, 2 * C, d["ss_off"], fault)
        s0, s1, ds0, ds1 = s[:, :C], s[:, C:], ds[:, :C], ds[:, C:]
        sc = s0 if fault == "no_plus1" else s0 + 1.0
        dsc = ds0 + EPS * sc.abs()
        a2 = a * sc
        b2 = (b + s1) * sc if fault == "shift_first" else b * sc + s1
        da, db = da * sc.abs() + a.abs() * dsc + EPS * a2.abs(), db * sc.abs() + b.abs() * dsc + ds1 + EPS * b2.abs()
        a, b = a2, b2
    return a, b, da, db


# layout cases: (B, C, G, nsplit); HW = 64 throughout (n = 64 cpg)
COEFF_LAYOUT = ([(2, 8, 1, ns) for ns in (1, 63, 64, 65, 511, 512, 513, 1024)] + [(2, 264, 1, 65)] +
                [(2, 64, 8, ns) for ns in (255, 256, 257)] + [(2, 1024, 8, 257)] +
                [(2, 64, 64, ns) for ns in (31, 32, 33)] + [(2, 1024, 64, 33)])
COEFF_FORMS = ("none", "a_img", "sampler0", "sampler_last", "a_img_row")


# ------------------------------------------------------------------------------------------------------------------------------
# cond_fold
# ------------------------------------------------------------------------------------------------------------------------------
def cond_fold_input(seed, B, with_b, with_row):
    """three entries of C = 64, 128, 512 at scattered offsets of rows ss_total = 1600 wide; flat holds their gains and biases"""
    g = gen(seed)
    entries = [(1400, 64, 700, 40),(16, 128, 2000, 900), (300, 512, 1028, 2200)]     # (ss_off, C, gamma offset, beta offset)
    W, T = 1600, 4
    rn = lambda *s: (0.4 * torch.randn(*s, generator=g)).float()
    d = dict(B=B, entries=entries, ss_total=W, flat=(1.0 + 0.5 * torch.randn(2800, generator=g)).float(),
             ss_a=rn(T, W) if with_row else rn(B, W), ss_a_stride=0 if with_row else W, row=T - 2 if with_row else None,
             row_stride=W if with_row else 0, ss_b=rn(B, W) if with_b else None, ss_b_stride=W if with_b else 0,
             pq=torch.full((B, W), -7.0, dtype=torch.float32))
    return d


def cond_fold_reference(d):
    """pq (B, ss_total) float64 after the launch and its tolerance: 0 (bit for bit) outside the entries"""
    ref, tol = d["pq"].double().clone(), torch.zeros(d["pq"].shape, dtype=torch.float64)
    flat = d["flat"].double()
    for off, C, go, bo in d["entries"]:
        s, ds = cond_rows(d, 2 * C, off)
        s0, s1, ds0, ds1 = s[:, :C], s[:, C:], ds[:, :C], ds[:, C:]
        sc = s0 + 1.0
        dsc = ds0 + EPS * sc.abs()
        gam, bet = flat[go:go + C][None], flat[bo:bo + C][None]
        P, Q = gam * sc, bet * sc + s1
        ref[:, off:off + C], ref[:, off + C:off + 2 * C] = P, Q
        tol[:, off:off + C] = gam.abs() * dsc + EPS * P.abs()
        tol[:, off + C:off + 2 * C] = bet.abs() * dsc + ds1 + EPS * Q.abs()
    return ref, tol


def zero_expected(zero_words, cleared=None):
    """the accumulator array of zero_words + 64 words after the launch (cleared: how many words a faulty loop clears)"""
    z = np.full(zero_words + 64, PATTERN, dtype=np.int64)
    z[:zero_words if cleared is None else max(cleared, 0)] = 0
    return z


# ------------------------------------------------------------------------------------------------------------------------------
# gn_fold: tables and the pass; affine_silu
# ------------------------------------------------------------------------------------------------------------------------------
def fold_tables(f, G, C, HW, images=None):
    """(A, Bc, dA, dB) (len(images), C): fold_coefficients with P, Q (C) shared or (B, C) per image"""
    B = f["acc"].shape[0]
    idx = torch.arange(B) if images is None else torch.tensor(images)
    if f["P"].dim() == 1:
        return fold_coefficients(f, G, C, HW, idx)
    parts = [fold_coefficients(dict(acc=f["acc"], P=f["P"][b], Q=f["Q"][b]), G, C, HW, torch.tensor([int(b)])) for b in idx]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(4))


def silu_err32(u, du):
    """float32 error of u / (1 + expf(-u)) at u + (an error of at most du)"""
    E = torch.exp(-u)
    share = torch.where(torch.isinf(E), torch.ones_like(E), E / (1.0 + E))
    return silu(u).abs() * (K_EXP * 2 * EPS * share + 2 * EPS) + 1.1 * du


def apply_reference(x, A, Bc, dA, dB, residual, dtype, scale=1.0):
    """out (B, C, HW) of SiLU(x A + Bc) + residual and its tolerance; x, residual: storage values; scale 2: a float32 evaluation of
    this reference is compared instead (its own error is at most the kernel's)"""
    bc = lambda t: t[:, :, None]
    if dtype == "bf16":
        s, ds = activation(x[..., None], A, Bc, dA, dB)
        s, ds = s[..., 0], ds[..., 0]
    else:
        u = x * bc(A) + bc(Bc)
        s, ds = silu(u), silu_err32(u, EPS * u.abs())
    ref, tol = s, ds
    if residual is not None:
        ref = s + residual
        tol = ds + (EPS * (s.abs() + residual.abs()) if dtype == "bf16" else EPS * ref.abs())
    tol = scale * tol
    if scale != 1.0:                              # the float32 evaluation forms u with two roundings, not an fmaf: e |x A| more
        tol = tol + 1.1 * EPS * (x * bc(A)).abs()
    if dtype == "bf16":
        tol = tol + half_ulp_bf16(ref.abs() + tol)
    return ref, tol


def apply_input(seed, B, C, HW, dtype, residual):
    g = gen(seed)
    x = stats_input(seed + 1, B, C, HW, dtype)
    r = store(torch.randn(B, C, HW, generator=g), dtype) if residual else None
    return x, (1.0 + 0.3 * torch.randn(B, C, generator=g)).float(), (0.5 * torch.randn(B, C, generator=g)).float(), r


# ------------------------------------------------------------------------------------------------------------------------------
# linear, sinusoidal
# ------------------------------------------------------------------------------------------------------------------------------
def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def gelu_err32(v, dv):
    er = torch.erf(v * math.sqrt(0.5))
    return (0.5 * v).abs() * (1.13 * EPS * (v * math.sqrt(0.5)).abs() + K_ERF * 2 * EPS * er.abs() + EPS * (1.0 + er).abs()) + EPS * gelu(v).abs() + 1.13 * dv


def act(v, kind):
    return silu(v) if kind == ACT_SILU else gelu(v) if kind == ACT_GELU else v


def act_err32(v, dv, kind):
    return silu_err32(v, dv) if kind == ACT_SILU else gelu_err32(v, dv) if kind == ACT_GELU else dv


def linear_input(seed, R, I, O, ldx=None, xoff=0, ldw=None, woff=0, bias=True, ldy=None, ycol=0, act_in=ACT_NONE, act_out=ACT_NONE):
    g = gen(seed)
    ldx, ldw, ldy = ldx or I, ldw or I, ldy or O
    return dict(R=R, I=I, O=O, ldx=ldx, xoff=xoff, ldw=ldw, woff=woff, ldy=ldy, ycol=ycol, act_in=act_in, act_out=act_out,
                x=torch.randn(R, ldx, generator=g).float(), W=(torch.randn(O, ldw, generator=g) * I ** -0.5).float(),
                bias=(0.3 * torch.randn(O, generator=g)).float() if bias else None, y=torch.full((R, ldy), -7.0, dtype=torch.float32))


def linear_reference(d, fault=None):
    """y (R, ldy) float64 after the launch and its tolerance (0 = untouched, bit for bit).  fault: "no_woff", "bias_anyway" (the
    bias of the other call form: 0.3 everywhere), "double_store", "drop_tail"."""
    R, I, O = d["R"], d["I"], d["O"]
    x = d["x"].double()[:, d["xoff"]:d["xoff"] + I]
    woff = 0 if fault == "no_woff" else d["woff"]
    w = d["W"].double()[:, woff:woff + I]
    if fault == "drop_tail":
        x, w = x[:, :256], w[:, :256]
    xa, dxa = act(x, d["act_in"]), act_err32(x, torch.zeros_like(x), d["act_in"])
    acc = xa @ w.T
    dacc = dxa @ w.abs().T + I * D53 * (xa.abs() @ w.abs().T) + EPS * acc.abs()
    if d["bias"] is not None:
        acc = acc + d["bias"].double()[None]
        dacc = dacc + EPS * acc.abs()
    elif fault == "bias_anyway":
        acc = acc + 0.3
    out, dout = act(acc, d["act_out"]), act_err32(acc, dacc, d["act_out"])
    ref, tol = d["y"].double().clone(), torch.zeros(d["y"].shape, dtype=torch.float64)
    c = d["ycol"]
    ref[:, c:c + O], tol[:, c:c + O] = out, dout
    if fault == "double_store" and c + O < d["ldy"]:
        ref[:, c + O] = out[:, O - 1]
    return ref, tol


# (R, I, O): every value of the issue's lists once, the three boundary triples together
LINEAR_SIZES = [(1, 1, 1), (63, 15, 2), (64, 16, 8), (65, 17, 9), (63, 255, 7), (64, 256, 8), (65, 257, 9), (1000, 520, 7), (65, 16, 1024)]


def sinus_input(R, dim, wide):
    half = dim // 2
    freqs = np.exp(np.arange(half, dtype=np.float32) * np.float32(-math.log(10000.0) / (half - 1))).astype(np.float32)
    base = [0, 1, 999] + ([2 ** 32 + 5] if wide else [])
    t = np.array([base[r % len(base)] + (r // len(base)) * 37 % 900 * (base[r % len(base)] == 1) for r in range(R)],
                 dtype=np.int64 if wide else np.int32)
    return t, freqs


def sinus_reference(t, freqs, fault=None):
    a = (t.astype(np.float32)[:, None] * freqs[None, :]).astype(np.float32).astype(np.float64)
    halves = [np.sin(a), np.cos(a)]
    if fault == "swap":
        halves = halves[::-1]
    ref = torch.from_numpy(np.concatenate(halves, axis=1))
    return ref, torch.full_like(ref, K_SIN * 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------------------------
# self-checks (CPU)
# ------------------------------------------------------------------------------------------------------------------------------
def shown(label, value):
    print(f"{label}: {value:.3g} tolerances")
    return value


@pytest.mark.parametrize("case", [c for c in STATS_CASES if c[4] <= 5000], ids=lambda c: f"{c[0]} {c[1]}")
def test_stats_reference_is_consistent(case):
    name, dtype, B, C, HW, G = case
    x = stats_input(1, B, C, HW, dtype)
    ns, sums, tol = stats_reference(x, G, dtype)
    assert sums.shape == (B, ns, G, 2) and bool((tol >= 0).all())
    # the slabs add up to the image's sums
    tot = torch.stack([x.reshape(B, G, -1).sum(dim=2), (x * x).reshape(B, G, -1).sum(dim=2)], dim=2)
    assert torch.allclose(sums.sum(dim=1), tot, rtol=1e-12, atol=1e-9)
    # a float32 accumulation of the same slabs (pairwise: shorter chains than the kernel's) is accepted
    v = F.pad(x, (0, ns * (-(-HW // ns)) - HW)).reshape(B, G, C // G, ns, -1).float()
    got = torch.stack([v.sum(dim=(2, 4)), (v * v).sum(dim=(2, 4))], dim=3).permute(0, 2, 1, 3)
    if dtype == "bf16":
        assert ratio(got, sums, tol) < 1.0


def test_a_slab_left_out_or_read_too_far_fails():
    for case in [c for c in STATS_CASES if "short last slab" in c[0]]:
        name, dtype, B, C, HW, G = case
        x = stats_input(STATS_CASES.index(case), B, C, HW, dtype)
        ns, sums, tol = stats_reference(x, G, dtype)
        assert shown(f"gn_stats {name} {dtype}: one slab left out", ratio(stats_reference(x, G, dtype, "drop_slab")[1], sums, tol)) > 1.0
        assert ns * (-(-HW // ns)) > HW
        far = stats_reference(x, G, dtype, "full_last_slab")[1]
        assert shown(f"gn_stats {name} {dtype}: the last slab read at full length", ratio(far[:-1], sums[:-1], tol[:-1])) > 1.0
        assert ratio(far[:, :-1], sums[:, :-1], tol[:, :-1]) == 0.0             # only the last slab notices


COEFF_FAULTS = [("drop_slab", "none", (2, 64, 8, 257)), ("no_ss_b", "sampler_last", (2, 64, 8, 257)), ("row0", "sampler_last", (2, 64, 8, 257)),
                ("row0", "a_img_row", (2, 64, 8, 257)), ("stride0", "a_img", (2, 64, 8, 257)), ("stride0", "a_img_row", (2, 64, 8, 257)),
                ("no_plus1", "a_img", (2, 64, 8, 257)), ("shift_first", "a_img", (2, 64, 8, 257)), ("eps_outside", "none", (2, 64, 8, 257)),
                ("c_mod_G", "none", (2, 64, 8, 257)), ("c_mod_G", "none", (2, 1024, 64, 33))]


@pytest.mark.parametrize("fault,form,layout", COEFF_FAULTS, ids=[f"{f[0]} {f[1]} C={f[2][1]}" for f in COEFF_FAULTS])
def test_coeff_mistakes_fail(fault, form, layout):
    B, C, G, ns = layout
    d = coeff_input(COEFF_LAYOUT.index(layout), B, C, G, 64, ns, form)
    a, b, ta, tb = coeff_reference(d)
    fa, fb = coeff_reference(d, fault)[:2]
    r = max(ratio(fa, a, ta), ratio(fb, b, tb))
    assert shown(f"gn_coeff {form} {layout}: {fault}", r) > 1.0
    if fault == "stride0":
        assert ratio(fa[:1], a[:1], ta[:1]) == 0.0                              # image 0 cannot tell


def test_coeff_edges():
    # the clamp: a constant image whose float32 slabs give a negative variance
    d = coeff_input(7, 2, 64, 8, 64, 16, "none", edge="constant")
    sl = d["slabs"].double().sum(dim=1)
    n = 64 * 8
    assert bool((sl[..., 1] / n - (sl[..., 0] / n) ** 2 < 0).all())
    a, b, ta, tb = coeff_reference(d)
    rstd = float(torch.tensor(1e-5, dtype=torch.float64) ** -0.5)
    assert torch.allclose(a, rstd * d["gamma"].double()[None].expand(2, -1), rtol=1e-15)
    fa, fb = coeff_reference(d, "no_clamp")[:2]
    assert shown("gn_coeff constant image: variance not clamped", max(ratio(fa, a, ta), ratio(fb, b, tb))) > 1.0
    fa, fb = coeff_reference(d, "eps_outside")[:2]
    assert shown("gn_coeff constant image: eps outside the root", max(ratio(fa, a, ta), ratio(fb, b, tb))) > 1.0
    # |mean| / std = 2^8: the reference resolves it: the tolerance stays a few float32 roundings of the coefficients
    d = coeff_input(8, 2, 64, 8, 64, 16, "none", edge="large_mean")
    a, b, ta, tb = coeff_reference(d)
    assert float((ta / a.abs()).max()) < 4 * EPS and float((tb / (b.abs() + 128.0 * a.abs())).max()) < 8 * EPS
    # and a float32 evaluation of the last steps from the float64 mean and rstd, as the kernel makes them, lies inside it
    sl = d["slabs"].double().sum(dim=1)
    mean = sl[..., 0] / n
    rs = ((sl[..., 1] / n - mean * mean).clamp(min=0.0) + 1e-5) ** -0.5
    a32 = rs.float().repeat_interleave(8, dim=1) * d["gamma"][None]
    b32 = d["beta"][None] - mean.float().repeat_interleave(8, dim=1) * a32
    assert max(ratio(a32, a, ta), ratio(b32, b, tb)) < 1.0


@pytest.mark.parametrize("form", COEFF_FORMS)
def test_a_float32_evaluation_of_the_conditioning_passes(form):
    d = coeff_input(3, 2, 64, 8, 64, 33, form)
    a, b, ta, tb = coeff_reference(d)
    plain = coeff_reference(dict(d, ss_a=None))
    a32, b32 = plain[0].float(), plain[1].float()
    if d["ss_a"] is not None:
        s, _ = cond_rows(dict(d, ss_b=None), 128, d["ss_off"])
        s = s.float()
        if d["ss_b"] is not None:
            s = s + d["ss_b"][:, 8:8 + 128]
        sc = s[:, :64] + 1.0
        a32, b32 = a32 * sc, (b32.double() * sc.double() + s[:, 64:].double()).float()
    assert max(ratio(a32, a, ta), ratio(b32, b, tb)) < 1.0


def test_cond_fold_reference_and_the_zero_loop():
    d = cond_fold_input(5, 3, True, True)
    ref, tol = cond_fold_reference(d)
    touched = tol > 0
    assert int(touched.sum()) == 3 * 2 * (64 + 128 + 512) and bool((ref[~touched] == -7.0).all())
    off, C, go, bo = d["entries"][0]
    s0 = d["ss_a"][2, off:off + C].double() + d["ss_b"][1, off:off + C].double()
    assert torch.allclose(ref[1, off:off + C], d["flat"][go:go + C].double() * (s0 + 1.0), rtol=1e-15)
    for zw in (500, 3 * 3 * 256, 3 * 3 * 256 + 1000):
        want = zero_expected(zw)
        assert int((want == 0).sum()) == zw and bool((want[zw:] == PATTERN).all())
        wrong = int((zero_expected(zw, cleared=zw - 64) != want).sum())
        assert shown(f"cond_fold zero_words {zw}: the last 64 words not cleared, wrong words", float(wrong)) == 64.0
        got = torch.from_numpy(zero_expected(zw, cleared=zw - 64))
        assert ratio(got, torch.from_numpy(want), torch.zeros(zw + 64)) == float("inf")


LINEAR_FAULTS = ["no_woff", "bias_anyway", "double_store", "drop_tail"]


def sampler_form(seed, R, e, O):
    """prg_sampler_run's call: the camera half of mlp_w, no bias, rows ldy wide at a column offset"""
    return linear_input(seed, R, e, O, ldx=2 * e, xoff=0, ldw=2 * e, woff=e, bias=False, ldy=O + 40, ycol=24, act_in=ACT_SILU)


@pytest.mark.parametrize("fault", LINEAR_FAULTS)
def test_linear_mistakes_fail(fault):
    # (the GPU test's inputs: seeds 100 + the index in LINEAR_SIZES, + 2 for the sampler's form)
    d = linear_input(106, 65, 257, 9, act_out=ACT_GELU) if fault == "drop_tail" else sampler_form(105, 65, 17, 9)
    ref, tol = linear_reference(d)
    bad = linear_reference(d, fault)[0]
    assert shown(f"linear: {fault}", ratio(bad, ref, tol)) > 1.0


@pytest.mark.parametrize("sizes", LINEAR_SIZES, ids=str)
def test_a_float32_linear_passes(sizes):
    R, I, O = sizes
    for d in (linear_input(1, R, I, O, act_out=ACT_GELU), linear_input(2, R, I, O), sampler_form(3, R, I, O)):
        ref, tol = linear_reference(d)
        x = d["x"][:, d["xoff"]:d["xoff"] + I]
        xa = F.silu(x) if d["act_in"] == ACT_SILU else x
        acc = (xa.double() @ d["W"][:, d["woff"]:d["woff"] + I].double().T).float()
        if d["bias"] is not None:
            acc = acc + d["bias"][None]
        got = d["y"].clone()
        got[:, d["ycol"]:d["ycol"] + O] = F.gelu(acc) if d["act_out"] == ACT_GELU else acc
        assert ratio(got, ref, tol) < 1.0


@pytest.mark.parametrize("wide", (0, 1))
def test_sinusoidal_reference(wide):
    for dim, R in ((4, 4), (6, 85), (64, 8), (130, 4)):
        t, freqs = sinus_input(R, dim, wide)
        assert {0, 1, 999} <= set(t.tolist())
        ref, tol = sinus_reference(t, freqs)
        assert ref.shape == (R, dim) and float(ref.abs().max()) <= 1.0
        assert shown(f"sinusoidal dim {dim}: cos and sin halves swapped", ratio(sinus_reference(t, freqs, "swap")[0], ref, tol)) > 1.0
        # numpy's float32 sin / cos of the same argument is inside the tolerance
        a = (t.astype(np.float32)[:, None] * freqs[None, :]).astype(np.float32)
        got = torch.from_numpy(np.concatenate([np.sin(a), np.cos(a)], axis=1))
        assert ratio(got, ref, tol) < 1.0
    if wide:
        t, freqs = sinus_input(4, 4, 1)
        low = sinus_reference((t & 0xFFFFFFFF).astype(np.int64), freqs)[0]
        ref, tol = sinus_reference(t, freqs)
        assert ratio(low, ref, tol) > 1.0                                       # the upper 32 bits matter


def test_apply_reference_special_values_and_emulation():
    for dtype in ("f32", "bf16"):
        x, A, Bc, r = apply_input(4, 2, 24 if dtype == "bf16" else 12, 50, dtype, True)
        z = torch.zeros(2, x.shape[1], dtype=torch.float64)
        ref, tol = apply_reference(x, A.double(), Bc.double(), z, z, r, dtype)
        u = (x * A.double()[:, :, None] + Bc.double()[:, :, None]).float()           # (fmaf: one rounding)
        got = store(F.silu(u) + r.float(), dtype)
        assert ratio(got, ref, tol) < 1.0
        # the next image's coefficients fail
        bad = apply_reference(x, A.double().roll(1, 0), Bc.double().roll(1, 0), z, z, r, dtype)[0]
        assert ratio(bad, ref, tol) > 1.0
        x[0, 0, 0] = float("-inf")
        A[0, 0] = 1.0
        ref, tol = apply_reference(x, A.double(), Bc.double(), z, z, None, dtype)
        assert math.isnan(float(ref[0, 0, 0])) and int(torch.isnan(ref).sum()) == 1


def test_fold_tables_per_image():
    g = gen(6)
    f = fold_inputs(g, 3, 8, 64, 256, poison=(1, 3))
    per = dict(acc=f["acc"], P=f["P"][None] * torch.tensor([[1.0], [2.0], [3.0]]), Q=f["Q"][None].expand(3, -1).contiguous())
    A, Bc, dA, dB = fold_tables(per, 8, 64, 256)
    A0 = fold_tables(f, 8, 64, 256)[0]
    ok = ~torch.isnan(A0)
    assert torch.allclose(A[ok], (A0 * torch.tensor([[1.0], [2.0], [3.0]]))[ok], rtol=1e-6)
    nan = torch.isnan(A)
    assert bool(nan[1, 24:32].all()) and int(nan.sum()) == 8
