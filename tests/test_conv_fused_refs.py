"""Float64 references, input families and derived tolerances for one bf16 convolution with the fused options of ConvLaunch
(prg_debug_conv_fused), and their self-checks on the CPU.  tests/test_gpu_conv_fused.py imports this module.

The operation, on operands first rounded to bf16 (x0, x1, w, residual; every coefficient, bias, gamma, beta stays float32):

    a   = cat[x0, x1]                       or, with a prologue,  bf16(SiLU(x0 * A[b, c] + Bc[b, c]))  (the padding ring stays 0)
    v   = conv_KxK(a, w) + bias             K = 3 pad 1 or K = 1 pad 0
    out = bf16(v)  |  bf16(v + r)  |  bf16(v + SiLU(r * A[b, c] + Bc[b, c]))
    S[b, g] = sum v,  Q[b, g] = sum v^2     over the pixels and channels of group g (the unrounded v)
    coefficients of GroupNorm:  mean = S / n, var = max(Q / n - mean^2, 0), rstd = (var + 1e-5)^-1/2,
                                a[b, c] = rstd gamma[c],  b[b, c] = beta[c] - mean a[b, c]
    folded coefficients (prologue or residual from fixed-point accumulators s, q): the same with S = s 2^-24, Q = q 2^-20 and
    (gamma, beta) = (P, Q); a negative q (the poison bit of gn_acc_add) gives NaN.

Tolerances (per element, e = 2^-24; none is fitted to an observed error):
  output      t32 = (n + 1) e (P + |bias|), n = (C0 + C1) K^2, P = conv(|a|, |w|): n float32 accumulations of exact bf16 x bf16
              products and the bias, which enters as one more addition (conv_ws, conv_epi.h) or as the accumulators' initial value
              (conv_c64, conv_w256): every partial sum is at most P + |bias|.
              + e (|v| + |r|) for the plain residual's addition; for the activated one the tail test's terms:
              |SiLU(u)| (|u| + 6) 2 e (v_exp_f32 and v_rcp_f32 at one ulp each, the roundings around them and of the exponent's
              argument) + 1.1 du (|SiLU'| <= 1.1) + e (|v| + |SiLU(u)|), where du = e |u| is the fmaf's rounding, plus, when the
              coefficients are folded in the kernel, |r| dA + dB with
                  dA = 4 e |A|                    (float) var and var + 1e-5f each round the argument by e -> e on rstd; v_rsq_f32 one
                                                  ulp = 2 e; the product rstd P one rounding
                  dB = 5 e |mean A| + e |B|       (float) mean, dA, and the fmaf's rounding
              (gn_fold_stats_raw in common.h; the same arithmetic in conv_epi.h:94-103, conv_c64.hip:442-449, conv_w256.hip:451-456
              and gn_coeff_acc_kernel).
              The bf16 store adds half a bf16 ulp taken at |ref| + t32.
  prologue    every kernel computes SiLU(fmaf(x, A, B)) as y * v_rcp_f32(1 + v_exp_f32(y * -log2 e)) (conv.hip:232 through
              Elem<bf16_t>::silu, conv_ws.hip:400, conv_c64.hip:426, conv_w256.hip:538): d = |SiLU(u)| (|u| + 6) 2 e + 1.1 du with du
              as above.  The operand is bf16 of that: an element whose float64 value lies within d of a bf16 rounding tie may round the
              other way, which moves it by one bf16 ulp; every other element is the reference's operand exactly.  The tolerance adds
              conv(mask ulp_bf16, |w|) and compares every output element.
  sums        v carries t32 (no rounding to bf16), a chain of `depth` float additions adds depth e sum |v|:
                  tol S = sum t32 + depth e sum |v|,    tol Q = sum (2 |v| t32 + t32^2 + e v^2) + depth e sum v^2
              (e v^2: the fmaf that squares and adds).  `depth` is read from each kernel's code: stat_depth() below.  The accumulator
              form rounds every partial to the fixed-point grid: + 2^-25 (S) and 2^-21 (Q) per partial.  When the conv fuses nothing
              and launch_gn_stats runs, the reference is the sums of the returned bf16 output and t32 = 0.
  coefficients  the sums' tolerance through mean, var (d var = dQ / n + 2 |mean| d mean + d mean^2) and rstd (monotone in var: its
              value at var - d var), then the float32 roundings: gn_coeff_kernel works in float64 and rounds mean and rstd once (e
              each), a = rstd gamma and b = beta - mean a round once each; the accumulator form is dA / dB above.
"""
import math

import pytest
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
LOG2E = 1.4426950408889634
GN_EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))     # the float32 constant of gn_fold_stats_raw
POISON = -(2 ** 63)                                             # kGnPoison: the sign bit of the sum-of-squares word


def bf16(x):
    return x.to(torch.bfloat16).double()


def half_ulp_bf16(v):
    """2^(E - 8) for 2^E <= v < 2^(E + 1) (bf16: 8 significant bits); 0 stays 0"""
    _, ex = torch.frexp(v.clamp(min=2.0 ** -120))
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), ex - 9), torch.zeros_like(v))


def silu(u):
    return u * torch.sigmoid(u)


def silu_err(u, du):
    """float32 error of y * rcp(1 + exp2(y * -log2 e)) at y = u + (an error of at most du)"""
    return silu(u).abs() * (u.abs() + 6.0) * 2 * EPS + 1.1 * du


def bc(t):
    return t[:, :, None, None]


# ------------------------------------------------------------------------------------------------------------------------------
# statistics: the longest chain of float additions a value passes through, kernel by kernel
# ------------------------------------------------------------------------------------------------------------------------------
def stat_depth(kernel, cpg, HW=0, C=0):
    per = cpg // 8
    lg = per.bit_length() - 1
    if kernel == "ws":
        # conv_ws.hip:708-714 a lane adds 2 pixel tiles x 4 registers; :734-741 six lane exchanges; :746-748 log2(cpg / 8) more
        return 8 + 6 + lg
    if kernel == "w256":
        # conv_w256.hip:295-305 four pixel tiles x 4 registers; :332-339 six exchanges; :341-343 log2(cpg / 8) more
        return 16 + 6 + lg
    if kernel == "c64":
        # conv_c64.hip:240-243 four pixel rows x 4 registers (pack_chunk); :302-308 six exchanges; :312-313 at most two more
        return 16 + 6 + min(lg, 2)
    if kernel in ("halo", "igemm"):
        # conv_epi.h:64-85 a lane adds 8 values in each of 4 passes, TM times (TM = 2 for the 8x32x64, 4x32x128 and 8x16x128 halo
        # tiles, 1 for the 128x64 gather tile); :149-152 three shuffles; :166-172 (cpg / 8) chunks x WAVES_M (at most 4) wave rows
        return 32 * (2 if kernel == "halo" else 1) + 3 + 4 * per
    if kernel == "gn_stats":
        # blocks.hip:43-50 a thread walks its slab's pixels with stride psub; :61-64 psub sub-lanes; :72-75 the group's channels
        psub = 256 // (C // 8)
        ns = max(1, min(1024, -(-HW // (psub * 8))))
        slab = -(-HW // ns)
        return -(-slab // psub) + psub + cpg
    raise ValueError(kernel)


# ------------------------------------------------------------------------------------------------------------------------------
# input families
# ------------------------------------------------------------------------------------------------------------------------------
def fold_inputs(g, B, G, C, HW, poison=None):
    """fixed-point accumulators of plausible statistics, and the folded gain / bias"""
    n = HW * (C // G)
    mean = 0.3 * torch.randn(B, G, generator=g).double()
    std = 0.5 + torch.rand(B, G, generator=g).double()
    acc = torch.stack([torch.round(mean * n * 2.0 ** 24), torch.round((std * std + mean * mean) * n * 2.0 ** 20)], dim=2).to(torch.int64)
    if poison is not None:
        acc[poison[0], poison[1], 1] |= POISON
    return dict(acc=acc, P=(1.0 + 0.3 * torch.randn(C, generator=g)).float(), Q=(0.5 * torch.randn(C, generator=g)).float())


def make_case(shape, K=3, groups=8, bias=True, pro=None, res=None, family="normal", seed=0, poison=None):
    """shape = (B, C0, C1, Cout, H, W).  pro: None, "tables", "fold";  res: None, "add", "tables", "fold".
    family: "normal" (every image its own amplitude and offset, every channel its own scale), "amplitude" (per-image rms from 2^-6
    to 2^9, |mean| <= rms), "zero_x0", "zero_x1", "border" (prologue A = 0, B = 0.7)"""
    B, C0, C1, Cout, H, W = shape
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    if family == "amplitude":
        rms = 2.0 ** torch.linspace(-6.0, 9.0, B) if B > 1 else torch.tensor([2.0 ** 9])
        amp, off = 0.8 * rms, 0.6 * rms * torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)
    else:
        amp = 0.5 + 1.5 * torch.rand(B, generator=g)
        off = amp * (torch.rand(B, generator=g) - 0.5)

    def source(C):
        scale = 0.75 + 0.5 * torch.rand(C, generator=g)
        return bf16((rn(B, C, H, W) * amp[:, None, None, None] + off[:, None, None, None]) * scale[None, :, None, None])

    d = dict(shape=shape, K=K, groups=groups, pro=pro, res=res, family=family)
    d["x0"] = source(C0)
    d["x1"] = source(C1) if C1 else None
    if family == "zero_x0":
        d["x0"].zero_()
    if family == "zero_x1":
        d["x1"].zero_()
    cin = C0 + C1
    d["w"] = bf16(rn(Cout, cin, K, K) * (cin * K * K) ** -0.5 * (0.5 + torch.rand(Cout, generator=g))[:, None, None, None])
    d["bias"] = (0.2 * rn(Cout)).float() if bias else None
    d["gamma"] = (1.0 + 0.3 * rn(Cout)).float()
    d["beta"] = (0.5 * rn(Cout)).float()
    if pro == "tables":
        d["pro_a"] = (1.0 + 0.3 * rn(B, C0)).float()
        d["pro_b"] = (0.5 * rn(B, C0)).float()
        if family == "border":
            d["pro_a"].zero_()
            d["pro_b"].fill_(0.7)
    if pro == "fold":
        d["fold"] = fold_inputs(g, B, groups, C0, H * W, poison)
    if res:
        d["residual"] = bf16(rn(B, Cout, H, W) * amp[:, None, None, None])
    if res == "tables":
        d["res_a"] = (1.0 + 0.3 * rn(B, Cout)).float()
        d["res_b"] = (0.5 * rn(B, Cout)).float()
    if res == "fold":
        d["fold"] = fold_inputs(g, B, groups, Cout, H * W, poison)
    return d


# ------------------------------------------------------------------------------------------------------------------------------
# float64 references and tolerances
# ------------------------------------------------------------------------------------------------------------------------------
def fold_coefficients(f, G, C, HW, idx):
    """(A, B, dA, dB) (len(idx), C) float64 of gn_fold_stats_raw + A = rstd P, B = fmaf(-mean, A, Q); NaN where poisoned"""
    cpg = C // G
    inv_n = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(HW), dtype=torch.float32) * torch.tensor(float(cpg), dtype=torch.float32)))
    acc = f["acc"][idx]
    s, q = acc[:, :, 0].double(), acc[:, :, 1].double()
    mean = s * 2.0 ** -24 * inv_n
    var = (q * 2.0 ** -20 * inv_n - mean * mean).clamp(min=0.0)
    rstd = (var + GN_EPS32) ** -0.5
    bad = acc[:, :, 1] < 0
    mean = torch.where(bad, torch.full_like(mean, float("nan")), mean).repeat_interleave(cpg, dim=1)
    rstd = torch.where(bad, torch.full_like(rstd, float("nan")), rstd).repeat_interleave(cpg, dim=1)
    A = rstd * f["P"].double()[None]
    Bc = f["Q"].double()[None] - mean * A
    return A, Bc, 4 * EPS * A.abs(), 5 * EPS * (mean * A).abs() + EPS * Bc.abs()


def activation(x, A, Bc, dA, dB):
    """(SiLU(u), its float32 error bound) for u = x A + Bc, per (image, channel) coefficients"""
    u = x * bc(A) + bc(Bc)
    du = EPS * u.abs() + x.abs() * bc(dA) + bc(dB)
    return silu(u), silu_err(u, du)


def bf16_tie_flip(s, delta):
    """per element: one bf16 ulp where s lies within delta of a bf16 rounding tie, else 0"""
    a = s.abs()
    ulp = 2 * half_ulp_bf16(a)
    r = a / ulp.clamp(min=2.0 ** -140)
    dist = ((r - r.floor()) - 0.5).abs() * ulp
    near = (dist <= delta) & (a > 0)
    return torch.where(near, 2 * half_ulp_bf16(a + delta), torch.zeros_like(a))


def zeros(n, C):
    return torch.zeros(n, C, dtype=torch.float64)


def conv_reference(d, images=None, dtype=torch.float64):
    """The output's reference and tolerance for the images `images` (all by default), with v and t32 for the statistics.  dtype
    float32: the convolutions run in float32 and t32 is doubled (the reference's own accumulation error is at most t32)."""
    B, C0, C1, Cout, H, W = d["shape"]
    K, G = d["K"], d["groups"]
    idx = torch.arange(B) if images is None else torch.tensor(sorted(set(images)))
    nb = len(idx)
    x0 = d["x0"][idx]
    wt = d["w"]
    conv = lambda a, w_: F.conv2d(a.to(dtype), w_.to(dtype), padding=K // 2).double()
    scale = 1.0 if dtype == torch.float64 else 2.0
    flip = None
    if d["pro"]:
        if d["pro"] == "tables":
            A, Bc, dA, dB = d["pro_a"][idx].double(), d["pro_b"][idx].double(), zeros(nb, C0), zeros(nb, C0)
        else:
            A, Bc, dA, dB = fold_coefficients(d["fold"], G, C0, H * W, idx)
        s, ds = activation(x0, A, Bc, dA, dB)
        a = bf16(s)
        flip = conv(bf16_tie_flip(s, ds), wt.abs())
    else:
        a = x0 if C1 == 0 else torch.cat([x0, d["x1"][idx]], dim=1)
    bias = d["bias"].double() if d["bias"] is not None else torch.zeros(Cout, dtype=torch.float64)
    v = conv(a, wt) + bias[None, :, None, None]
    P = conv(a.abs(), wt.abs()) + bias.abs()[None, :, None, None]
    n = (C0 + C1) * K * K
    t32 = scale * (n + 1) * EPS * P
    if flip is not None:
        t32 = t32 + flip
    ref, tout = v, t32
    if d["res"] == "add":
        r = d["residual"][idx]
        ref = v + r
        tout = t32 + EPS * (v.abs() + r.abs())
    elif d["res"]:
        r = d["residual"][idx]
        if d["res"] == "tables":
            A, Bc, dA, dB = d["res_a"][idx].double(), d["res_b"][idx].double(), zeros(nb, Cout), zeros(nb, Cout)
        else:
            A, Bc, dA, dB = fold_coefficients(d["fold"], G, Cout, H * W, idx)
        s, ds = activation(r, A, Bc, dA, dB)
        ref = v + s
        tout = t32 + ds + EPS * (v.abs() + s.abs())
    return dict(images=idx, ref=ref, tol=tout + half_ulp_bf16(ref.abs() + tout), v=v, t32=t32)


def reference(d, images=None, dtype=torch.float64, kernel=None, partials=0, from_output=None, core=None, depth=None):
    """conv_reference (or a `core` it returned earlier) plus the statistics.  kernel / partials: the statistics producer
    (stat_depth) and, for the accumulator form, its partial count per image group; None = no statistics.  from_output: the
    (len(images), Cout, H, W) bf16 output itself when launch_gn_stats produced the sums (kernel = "gn_stats").  depth: the chain
    length itself, for a producer stat_depth does not know (the float kernels: tests/test_conv_fused_f32_refs.py)."""
    out = dict(core if core is not None else conv_reference(d, images, dtype))
    if kernel is None:
        return out
    B, C0, C1, Cout, H, W = d["shape"]
    G = d["groups"]
    v, t32, nb = out["v"], out["t32"], len(out["images"])
    cpg = Cout // G
    npg = H * W * cpg
    if kernel == "gn_stats":
        v, t32 = from_output, torch.zeros_like(from_output)
    depth = stat_depth(kernel, cpg, H * W, Cout) if depth is None else depth
    grp = lambda t: t.reshape(nb, G, cpg * H * W).sum(dim=2)
    S, Q = grp(v), grp(v * v)
    tS = grp(t32) + depth * EPS * grp(v.abs()) + partials * 2.0 ** -25
    tQ = grp(2 * v.abs() * t32 + t32 * t32 + EPS * v * v) + depth * EPS * Q + partials * 2.0 ** -21
    out.update(sums=torch.stack([S, Q], dim=2), sums_tol=torch.stack([tS, tQ], dim=2))
    # GroupNorm coefficients and what the sums' tolerance and the float32 steps leave of them
    mean, dmean = S / npg, tS / npg
    var = (Q / npg - mean * mean).clamp(min=0.0)
    dvar = tQ / npg + 2 * mean.abs() * dmean + dmean * dmean
    eps = GN_EPS32 if partials else 1e-5
    rstd = (var + eps) ** -0.5
    drstd = ((var - dvar).clamp(min=0.0) + eps) ** -0.5 - rstd
    ch = lambda t: t.repeat_interleave(cpg, dim=1)
    gam, bet = d["gamma"].double()[None], d["beta"].double()[None]
    A = ch(rstd) * gam
    Bc = bet - ch(mean) * A
    if partials:      # gn_fold_stats_raw + gn_coeff_acc_kernel
        dA = gam.abs() * ch(drstd) + 4 * EPS * A.abs()
        dB = A.abs() * ch(dmean) + ch(mean.abs()) * gam.abs() * ch(drstd) + 5 * EPS * (ch(mean) * A).abs() + EPS * Bc.abs()
    else:             # gn_coeff_kernel (blocks.hip:221-243): float64 to (float) mean, (float) rstd, then two float32 roundings each
        dA = gam.abs() * (ch(drstd) + EPS * ch(rstd)) + EPS * A.abs()
        dB = A.abs() * (ch(dmean) + EPS * ch(mean.abs())) + ch(mean.abs()) * dA + EPS * (ch(mean) * A).abs() + EPS * Bc.abs()
    out.update(coef_a=A, coef_b=Bc, coef_a_tol=dA, coef_b_tol=dB)
    return out


def ratios(label, got, ref, show=True):
    """largest error / tolerance of every quantity both sides hold; NaN / Inf in `got` counts as infinite"""
    idx = ref["images"]
    pairs = [("out", got["out"][idx], ref["ref"], ref["tol"])]
    if "sums" in ref:
        pairs += [("sums", got["sums"][idx], ref["sums"], ref["sums_tol"]), ("coef_a", got["coef_a"][idx], ref["coef_a"], ref["coef_a_tol"]),
                  ("coef_b", got["coef_b"][idx], ref["coef_b"], ref["coef_b_tol"])]
    res = {}
    for name, g_, r_, t_ in pairs:
        g_ = g_.double()
        q = (g_ - r_).abs() / t_
        inf = torch.full_like(q, float("inf"))
        q = torch.where(torch.isfinite(g_), q, inf)
        q = torch.where(g_ == r_, torch.zeros_like(q), q)
        q = torch.where(torch.isnan(r_), torch.where(torch.isnan(g_), torch.zeros_like(q), inf), q)    # a poisoned group: NaN expected
        res[name] = float(q.max())
    if show:
        print(f"{label}: largest error / tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    return res


# ------------------------------------------------------------------------------------------------------------------------------
# a float32 emulation of the formulas: the stand-in kernel of the self-checks below
# ------------------------------------------------------------------------------------------------------------------------------
def f32(x):
    return x.to(torch.float32)


def fma32(x, a, b):
    return f32(x.double() * a.double() + b.double())        # (an exact product and one rounding, up to a double rounding)


def silu32(y):
    return y * (1.0 / (1.0 + torch.exp2(y * f32(torch.tensor(-LOG2E)))))


def fold32(f, G, C, HW):
    cpg = C // G
    inv_n = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(HW), dtype=torch.float32) * torch.tensor(float(cpg), dtype=torch.float32))
    s, q = f["acc"][:, :, 0].double(), f["acc"][:, :, 1].double()
    m = s * 2.0 ** -24 * inv_n.double()
    var = (q * 2.0 ** -20 * inv_n.double() - m * m).clamp(min=0.0)
    mean = f32(m).repeat_interleave(cpg, dim=1)
    rstd = torch.rsqrt(f32(var) + torch.tensor(1e-5, dtype=torch.float32)).repeat_interleave(cpg, dim=1)
    A = rstd * f["P"][None]
    return A, fma32(-mean, A, f["Q"][None].expand_as(A))


def emulate(d, nslab=0, acc=False, fault=None):
    """out, sums, coefficients as a kernel accumulating in float32 would give them.  nslab > 0: statistics in nslab row bands per
    image (H % nslab == 0), as fixed-point accumulators when `acc`.  fault: "drop_slab", "swap_sources", "activate_ring",
    "next_image_coeffs": the four mistakes the checks must catch."""
    B, C0, C1, Cout, H, W = d["shape"]
    K, G = d["K"], d["groups"]
    nxt = (lambda t: torch.roll(t, -1, dims=0)) if fault == "next_image_coeffs" else (lambda t: t)
    pad = K // 2
    if d["pro"]:
        A, Bc = (d["pro_a"], d["pro_b"]) if d["pro"] == "tables" else fold32(d["fold"], G, C0, H * W)
        A, Bc = nxt(A), nxt(Bc)
        a = f32(bf16(silu32(fma32(f32(d["x0"]), bc(A).expand_as(d["x0"]), bc(Bc).expand_as(d["x0"])))))
        if fault == "activate_ring":
            ring = f32(bf16(silu32(Bc)))
            full = bc(ring).expand(B, C0, H + 2, W + 2).clone()
            full[:, :, 1:-1, 1:-1] = a
            a, pad = full, 0
    else:
        srcs = [d["x0"]] + ([d["x1"]] if C1 else [])
        if fault == "swap_sources":
            srcs = srcs[::-1]
        a = f32(torch.cat(srcs, dim=1))
    v = F.conv2d(a, f32(d["w"]), padding=pad)
    if d["bias"] is not None:
        v = v + d["bias"][None, :, None, None]
    o = v
    if d["res"] == "add":
        o = v + f32(d["residual"])
    elif d["res"]:
        A, Bc = (d["res_a"], d["res_b"]) if d["res"] == "tables" else fold32(d["fold"], G, Cout, H * W)
        A, Bc = nxt(A), nxt(Bc)
        r = f32(d["residual"])
        o = v + silu32(fma32(r, bc(A).expand_as(r), bc(Bc).expand_as(r)))
    got = dict(out=bf16(o))
    if not nslab:
        return got
    cpg, rows = Cout // G, H // nslab
    vs = v.reshape(B, G, cpg, nslab, rows * W).permute(0, 3, 1, 2, 4).reshape(B, nslab, G, cpg * rows * W)
    slabs = torch.stack([vs.sum(dim=3), (vs * vs).sum(dim=3)], dim=3)                 # (B, nslab, G, 2) float32
    if fault == "drop_slab":
        slabs[:, nslab // 2] = 0.0
    npg = H * W * cpg
    if acc:
        fixed = torch.round(slabs.double() * torch.tensor([2.0 ** 24, 2.0 ** 20])).to(torch.int64).sum(dim=1)
        got["sums"] = fixed.double() * torch.tensor([2.0 ** -24, 2.0 ** -20])
        A, Bc = fold32(dict(acc=fixed, P=d["gamma"], Q=d["beta"]), G, Cout, H * W)
    else:
        got["sums"] = slabs.double().sum(dim=1)
        mean = got["sums"][:, :, 0] / npg
        var = (got["sums"][:, :, 1] / npg - mean * mean).clamp(min=0.0)
        mean32, rstd32 = f32(mean).repeat_interleave(cpg, dim=1), f32((var + 1e-5) ** -0.5).repeat_interleave(cpg, dim=1)
        A = rstd32 * d["gamma"][None]
        Bc = d["beta"][None] - mean32 * A
    got.update(coef_a=A.double(), coef_b=Bc.double())
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# self-checks (CPU)
# ------------------------------------------------------------------------------------------------------------------------------
SMALL = (3, 16, 16, 16, 8, 16)         # (B, C0, C1, Cout, H, W), groups 2
FAMILIES = [
    ("two sources", dict(shape=SMALL, groups=2), dict()),
    ("two sources, no bias", dict(shape=SMALL, groups=2, bias=False), dict()),
    ("zero x0", dict(shape=SMALL, groups=2, family="zero_x0"), dict()),
    ("zero x1", dict(shape=SMALL, groups=2, family="zero_x1"), dict()),
    ("amplitude, slabs", dict(shape=(6, 16, 16, 16, 8, 16), groups=2, family="amplitude"), dict(nslab=4)),
    ("amplitude, accumulators", dict(shape=(6, 16, 16, 16, 8, 16), groups=2, family="amplitude"), dict(nslab=4, acc=True)),
    ("slabs", dict(shape=SMALL, groups=2), dict(nslab=8)),
    ("accumulators", dict(shape=SMALL, groups=1), dict(nslab=2, acc=True)),
    ("table prologue", dict(shape=(3, 16, 0, 16, 8, 16), groups=2, pro="tables"), dict()),
    ("table prologue, border", dict(shape=(3, 16, 0, 16, 8, 16), groups=2, pro="tables", family="border"), dict()),
    ("fold prologue", dict(shape=(3, 16, 0, 16, 8, 16), groups=2, pro="fold"), dict(nslab=4)),
    ("1x1", dict(shape=(3, 16, 8, 16, 6, 6), K=1, groups=2), dict()),
    ("1x1 add", dict(shape=(3, 16, 8, 16, 6, 6), K=1, groups=2, res="add"), dict()),
    ("1x1 tables", dict(shape=(3, 16, 8, 16, 6, 6), K=1, groups=2, res="tables"), dict()),
    ("1x1 fold", dict(shape=(3, 16, 8, 16, 6, 6), K=1, groups=2, res="fold"), dict()),
]


def check_emulation(d, fault=None, nslab=0, acc=False, label=""):
    # (the stand-in's statistics are held to the shortest chain of any kernel, conv_ws's: torch's float32 sums are pairwise)
    got = emulate(d, nslab=nslab, acc=acc, fault=fault)
    ref = reference(d, kernel="ws" if nslab else None, partials=nslab if acc else 0)
    return ratios(label, got, ref)


@pytest.mark.parametrize("name,case,stats", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_faithful_emulation_passes(name, case, stats):
    d = make_case(seed=11, **case)
    r = check_emulation(d, label=name, **stats)
    assert max(r.values()) < 1.0, r
    # the float32-convolution form of the reference (used for the large batches on the GPU) accepts it too
    ref32 = reference(d, dtype=torch.float32, kernel="ws" if stats else None, partials=stats.get("nslab", 0) if stats.get("acc") else 0)
    r32 = ratios(name + " (float32 reference)", emulate(d, **stats), ref32)
    assert max(r32.values()) < 1.0, r32
    # and a subset of the images is the same reference
    sub = reference(d, images=[0, d["shape"][0] - 1])
    full = reference(d)
    last = d["shape"][0] - 1
    assert torch.allclose(sub["ref"], full["ref"][[0, last]], rtol=1e-12, atol=0) and torch.allclose(sub["tol"], full["tol"][[0, last]], rtol=1e-12, atol=0)


@pytest.mark.parametrize("acc", (False, True), ids=("slabs", "accumulators"))
def test_a_dropped_slab_fails(acc):
    # 128 slabs per image group: one missing changes rstd by about 0.4 %
    d = make_case((2, 16, 16, 16, 128, 8), groups=2, seed=5)
    ok = check_emulation(d, nslab=128, acc=acc, label="128 slabs")
    bad = check_emulation(d, fault="drop_slab", nslab=128, acc=acc, label="one slab of 128 dropped")
    assert max(ok.values()) < 1.0
    assert bad["out"] < 1.0 and bad["sums"] > 1.0 and bad["coef_a"] > 1.0, bad


def test_swapped_sources_fail():
    d = make_case(SMALL, groups=2, seed=6)
    assert check_emulation(d, fault="swap_sources", label="sources swapped")["out"] > 1.0
    for fam in ("zero_x0", "zero_x1"):
        assert check_emulation(make_case(SMALL, groups=2, family=fam, seed=6), fault="swap_sources", label=f"sources swapped, {fam}")["out"] > 1.0


@pytest.mark.parametrize("pro", ("tables", "fold"))
def test_an_activated_padding_ring_fails(pro):
    fams = ("normal", "border") if pro == "tables" else ("normal",)
    for fam in fams:
        d = make_case((3, 16, 0, 16, 8, 16), groups=2, pro=pro, family=fam, seed=7)
        got = emulate(d, fault="activate_ring")
        ref = reference(d)
        r = ratios(f"padding ring activated, {pro}, {fam}", got, ref)
        assert r["out"] > 1.0
        # only the edge pixels notice
        inner = ((got["out"] - ref["ref"]).abs() / ref["tol"])[:, :, 1:-1, 1:-1]
        assert float(inner.max()) < 1.0


@pytest.mark.parametrize("mode", ("pro tables", "pro fold", "res tables", "res fold"))
def test_the_next_images_coefficients_fail(mode):
    kind, how = mode.split()
    if kind == "pro":
        d = make_case((3, 16, 0, 16, 8, 16), groups=2, pro=how, seed=8)
    else:
        d = make_case((3, 16, 8, 16, 6, 6), K=1, groups=2, res=how, seed=8)
    assert check_emulation(d, label=mode)["out"] < 1.0
    assert check_emulation(d, fault="next_image_coeffs", label=mode + ", coefficients of image b + 1")["out"] > 1.0


def test_poisoned_accumulators_give_nan_coefficients():
    d = make_case((3, 16, 8, 16, 6, 6), K=1, groups=2, res="fold", seed=9, poison=(1, 1))
    ref = reference(d)["ref"]
    bad = torch.isnan(ref)
    assert bool(bad[1, 8:].all()) and int(bad.sum()) == 8 * 36
    # a finite value where NaN is expected counts as a failure, NaN there as agreement
    full = reference(d)
    got = dict(out=torch.nan_to_num(ref, nan=0.0))
    assert ratios("poisoned group answered with numbers", got, full)["out"] == float("inf")
    assert ratios("poisoned group answered with NaN", dict(out=ref), full)["out"] == 0.0


def test_tie_mask_marks_only_near_ties():
    s = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 1e-6, 1.0 + 2.0 ** -7, 0.0, -(3.0 + 2.0 ** -7), 1.0 + 2.0 ** -8 - 1e-9], dtype=torch.float64)
    f = bf16_tie_flip(s, torch.full_like(s, 1e-7))
    assert f.tolist() == [2.0 ** -7, 0.0, 0.0, 0.0, 2.0 ** -6, 2.0 ** -7]


def test_stat_depths():
    assert stat_depth("ws", 8) == 14 and stat_depth("ws", 64) == 17
    assert stat_depth("w256", 16) == 23 and stat_depth("c64", 8) == 22 and stat_depth("c64", 64) == 24
    assert stat_depth("halo", 8) == 71 and stat_depth("igemm", 8) == 39
    assert stat_depth("gn_stats", 8, HW=144, C=64) == 5 + 32 + 8
    assert math.isclose(GN_EPS32, 1e-5, rel_tol=1e-7) and GN_EPS32 != 1e-5
