"""Float64 references, input families and derived tolerances for one float32-storage convolution (PRG_F16X3: the split-f16 kernels
of conv_split.hip / conv_split512.hip; PRG_F32: the exact kernels of conv.hip with T = float) with the fused options of ConvLaunch
(prg_debug_conv_fused with storage 1 / 2), and their self-checks on the CPU.  tests/test_gpu_conv_fused_f32.py imports this module;
the formulas shared with bf16 (silu_err, the sums' and the coefficients' tolerances) are tests/test_conv_fused_refs.py's own.

The operation is that module's without any rounding to bf16: the operands are the float32 values themselves (x0, x1, w, residual,
every coefficient), and the output is the float32 v (+ residual), never rounded again.

Tolerances (per element, e = 2^-24; P = conv(|a|, |w|); none is fitted to an observed error):
  output, f16x3
      split   each operand becomes hi + lo, hi = f16(x), lo = f16(x - hi) (conv_split_common.h:13-35, weights_host.cpp f16_hi_lo), and
              the lo * lo product is dropped (conv_split.hip:4-8, mma3 :31-35).  A normal lo leaves 2^-22 |x|; a subnormal one leaves its
              half step 2^-25 (f16 subnormals are kept by the instruction, conv_split.hip:4), so  da <= 2^-22 |a| + 2^-25.  The packer
              multiplies every output channel's weights by the power of two that brings max |w| into [2^9, 2^10)
              (weights_host.cpp:209-224), so in units of the weight the floor is 2^-25 / 2^9:  dw <= 2^-22 |w| + 2^-34 max_c |w|; the kernels
              undo the factor exactly (conv_split.hip:359-365, :787, :1171, :1370-1378; conv_split512.hip:298).  With |lo| <= 2^-11 |x|
              (+ the floors):  |a w - (a_hi w_hi + a_hi w_lo + a_lo w_hi)| <= da |w| + |a| dw + |a_lo| |w_lo|, summed:
                  t_split = 3 * 2^-22 (1 + 2^-10) P + 2^-25 (1 + 2^-10) conv(1, |w|) + 2^-34 conv(|a|, 1) max_c |w|
              (conv(1, .) over the real pixels: the padding ring is an exact zero whose halves are zero).
      chain   the products of two f16 values are exact in float32; the matrix pipe adds the 9 taps x 32 channels = 288 terms of a
              32-channel chunk into one accumulator set, which is then added to a second float32 set (conv_split.hip:333-338 halo,
              :740-747 ws, the same in the p64 kernel; conv_split512.hip:250), and the epilogue adds the bias once (tot * scale + bias,
              the product exact):  t_chain = (288 + chunks + 1) e (P + |bias|), chunks = ceil((C0 + C1) / 32).  The gather kernel
              (conv_igemm_split_kernel, 3x3 below a halo tile and every 1x1) flushes every 8 steps of 32 channels
              (conv_split.hip:1357): (256 + ceil(K^2 chunks / 8) + 1) e (P + |bias|).
              Cross-check with the conv-level bound of tests/test_gpu_f16x3.py (2^-19 P + 2^-22 max |ref|) at K = 576: the split part
              alone is 12.01 e P against its 32 e P; with the chain (291 e P) it is 303 e P, nine times LOOSER.  The conv-level bound has no
              term for the accumulation at all: it holds there because 288 float32 roundings of either sign average out, not
              because they must.  This module's chain term is the worst case of every rounding, which no input can exceed (the
              matrix pipe rounds at most once per product term); what it costs in sharpness is measured by the planted fault
              "lo half dropped" below.
  output, fp32  v_mfma_f32_32x32x2_f32 products are exact; the 32 terms of one (tap, 32-channel chunk) step are one float32 chain,
              and the steps are added in float64 (conv.hip:69-115 Wide<float>, :252 / :272; the gather kernel 16 terms, :650), rounded
              to float32 once (:108-115) and the bias added in the epilogue (conv_epi.h:71):  t = (32 + 2) e (P + |bias|) instead of
              (n + 1) e (P + |bias|).
  prologue    the operand is the float32 value of SiLU(fmaf(x, A, B)): fast_silu (common.h:65-67: y * v_rcp_f32(1 + v_exp_f32(y * -log2 e)))
              in every split kernel (conv_split.hip:198, :590, :983; conv_split512.hip:116-117), Elem<float>::silu = y / (1 + expf(-y))
              in conv.hip:232.  silu_err(u, e |u|) covers both (expf and the division are at least as accurate as the two one-ulp
              instructions).  No rounding tie can be masked: d = silu_err propagates as conv(d, |w|), and the split's da is taken at
              |a| + d.  The padding ring is exactly zero (conv_split.hip:196-205 under the in-image test; conv.hip:230 hsrc >= 0).
  epilogues   (1x1, the shared transposing epilogue conv_epi.h:85-127)  plain residual: + e (|v| + |r|); activated residual
              SiLU(fmaf(r, A, B)) with Elem<float>::silu: + silu_err(u, e |u|) + e (|v| + |SiLU(u)|).
  sums        the bf16 module's formulas, tol S = sum t + depth e sum |v|, tol Q = sum (2 |v| t + t^2 + e v^2) + depth e sum v^2, with
              `depth` = the float32 additions a value passes before the sums continue in float64, + 1 for the rounding of the slab:
                  split halo            16 + 1   conv_split.hip:378-389 a lane adds its 16 pixels, :396-424 float64 from there
                  split ws / p64 / w512 32 + 1   conv_split.hip:780-797, :1163-1178, conv_split512.hip:289-311: 2 x 16 registers
                  conv_epi.h path        1 + 1   (T = float: conv.hip's halo and gather kernels and conv_igemm_split_kernel)
                                                 StatAcc<float> = double from the first addition (conv_epi.h:12-16, :79-83), one unit
                                                 for the float64 chain of at most 2^29 terms, one for the (float) of the slab (:172-173)
                  launch_gn_stats<float> 1 + 1   blocks.hip:14-20 Acc<float> = double throughout, (float) at :77-78; its reference is
                                                 the sums of the returned output itself, t = 0
              The same tolerance restricted to one slab's pixels holds for that slab.  Slab index of a pixel (y, x), slab_map():
                  split halo, conv.hip halo   (y / th) tiles_x + x / tw                              conv_split.hip:421-422, conv.hip:285-286
                  split ws                    ((y / 8) tiles_x + x / 16) 2 + (y % 8) / 4            conv_split.hip:809-810 (wm = rows 4 wm ..)
                  split w512                  the same map: ((2 ty + wm) tiles_x + tx) 2 + half      conv_split512.hip:286-320
                  split p64                   ((y / 16) tiles_x + x / 16) 4 + (y % 16) / 4           conv_split.hip:1191 (wave = rows 4 wave ..)
                  gather kernels              (y W + x) / BM                                         conv_split.hip:1382-1384, conv.hip igemm
  coefficients  launch_gn_coeff only (there are no accumulators in these modes): the bf16 module's non-accumulator formulas.

Planted faults (CPU, emulate32): largest error / tolerance each lands at, smallest .. largest over the tile shapes of TILES:
  one slab left out                         sums 113 (p64: 1 of 16 slabs) .. 1.7e4, that slab 1.7e3 .. 1.7e4, coef_a 109 .. 2.0e7
  slab indices of two wave rows swapped     slabs 336 .. 3.3e3; the sums and coefficients stay below 7e-4 and 3e-3: only the slab-wise
                                            comparison sees it
  sources swapped                           out 1.8e4 .. 3.0e4 (f16x3), 1.6e5 .. 2.7e5 (fp32), zero sources included
  prologue applied to the padding ring      out 7.4e3 .. 1.6e4 (f16x3), 5.8e4 .. 1.1e5 (fp32), edge pixels only
  image b + 1's coefficient row             out 1.3e4 .. 1.8e4 (f16x3), 8.0e4 .. 9.1e4 (fp32); 1x1 tables 3.8e4 / 2.7e5
  lo half of the activations dropped        out 2.45 .. 2.97 over the six f16x3 tile shapes (K = 1080, 1152), above 1 on the 1x1 shapes; a
                                            bf16-grade tolerance ((n + 1) e P and half a bf16 ulp) passes the same fault at 0.53 .. 0.65
  one 32-channel chunk of x1 skipped        out 5.9e3 .. 7.9e3 (f16x3), 5.1e4 .. 7.1e4 (fp32)
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from test_conv_fused_refs import EPS, bc, f32, fma32, ratios, reference, silu, silu32, silu_err

F16X3, F32 = 1, 2                      # prg_conv_fused.storage
SPLIT_TILE_KERNELS = ("split_halo", "split_ws", "split_p64", "split_w512")
STAT_DEPTH = {"split_halo": 17, "split_ws": 33, "split_p64": 33, "split_w512": 33, "split_igemm": 2, "halo": 2, "igemm": 2, "gn_stats": 2}


def storage_of(kernel):
    return F16X3 if kernel.startswith("split") else F32


def chain_terms(kernel, cin, K):
    """the factor of e (P + |bias|): the longest float32 chain of the accumulation, its flushes and the bias"""
    chunks = -(-cin // 32)
    if kernel in SPLIT_TILE_KERNELS:
        return 288 + chunks + 1
    if kernel == "split_igemm":
        return 256 + -(-(K * K * chunks) // 8) + 1
    if kernel in ("halo", "igemm"):
        return 32 + 2
    raise ValueError(kernel)


def slab_map(kernel, tile, H, W):
    """(slab index of every pixel (H * W,), slabs per image) of a kernel that fuses the statistics"""
    y, x = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    if kernel in ("split_halo", "halo"):
        th, tw = tile[0], tile[1]
        m, n = (y // th) * (W // tw) + x // tw, (H // th) * (W // tw)
    elif kernel in ("split_ws", "split_w512"):
        m, n = ((y // 8) * (W // 16) + x // 16) * 2 + (y % 8) // 4, (H // 8) * (W // 16) * 2
    elif kernel == "split_p64":
        m, n = ((y // 16) * (W // 16) + x // 16) * 4 + (y % 16) // 4, (H // 16) * (W // 16) * 4
    elif kernel in ("split_igemm", "igemm"):
        m, n = (y * W + x) // tile[0], (H * W) // tile[0]
    else:
        raise ValueError(kernel)
    return m.reshape(-1), n


# ------------------------------------------------------------------------------------------------------------------------------
# input families
# ------------------------------------------------------------------------------------------------------------------------------
def make_case32(shape, K=3, groups=8, bias=True, pro=None, res=None, family="normal", seed=0, distinct=None):
    """shape = (B, C0, C1, Cout, H, W); float32 values (held as float64).  pro: None, "tables";  res: None, "add", "tables".
    family: "normal", "amplitude" (per-image rms 2^-6 .. 2^9), "tiny" (rms 2^-16: below the f16 normal range, the hi halves are
    subnormal), "zero_x0", "zero_x1", "border" (prologue A = 0, B = 0.7).  distinct = n: only n images are drawn (shape[0] becomes
    n); expand() makes the launch of B images out of them."""
    B, C0, C1, Cout, H, W = shape
    launch_B = B
    if distinct:
        B = distinct
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    r32 = lambda t: t.float().double()
    if family == "amplitude":
        rms = 2.0 ** torch.linspace(-6.0, 9.0, B) if B > 1 else torch.tensor([2.0 ** 9])
        amp, off = 0.8 * rms, 0.6 * rms * torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)
    elif family == "tiny":
        amp, off = torch.full((B,), 0.8 * 2.0 ** -16), 0.6 * 2.0 ** -16 * torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)
    else:
        amp = 0.5 + 1.5 * torch.rand(B, generator=g)
        off = amp * (torch.rand(B, generator=g) - 0.5)

    def source(C):
        scale = 0.75 + 0.5 * torch.rand(C, generator=g)
        return r32((rn(B, C, H, W) * amp[:, None, None, None] + off[:, None, None, None]) * scale[None, :, None, None])

    d = dict(shape=(B, C0, C1, Cout, H, W), launch_B=launch_B, K=K, groups=groups, pro=pro, res=res, family=family)
    d["x0"] = source(C0)
    d["x1"] = source(C1) if C1 else None
    if family == "zero_x0":
        d["x0"].zero_()
    if family == "zero_x1":
        d["x1"].zero_()
    cin = C0 + C1
    d["w"] = r32(rn(Cout, cin, K, K) * (cin * K * K) ** -0.5 * (0.5 + torch.rand(Cout, generator=g))[:, None, None, None])
    d["bias"] = (0.2 * rn(Cout)).float() if bias else None
    d["gamma"] = (1.0 + 0.3 * rn(Cout)).float()
    d["beta"] = (0.5 * rn(Cout)).float()
    if pro == "tables":
        d["pro_a"] = (1.0 + 0.3 * rn(B, C0)).float()
        d["pro_b"] = (0.5 * rn(B, C0)).float()
        if family == "border":
            d["pro_a"].zero_()
            d["pro_b"].fill_(0.7)
    if res:
        d["residual"] = r32(rn(B, Cout, H, W) * amp[:, None, None, None])
    if res == "tables":
        d["res_a"] = (1.0 + 0.3 * rn(B, Cout)).float()
        d["res_b"] = (0.5 * rn(B, Cout)).float()
    return d


def expand(d):
    """the launch of launch_B images: image b is a copy of image b % n, its coefficient rows likewise"""
    n, B = d["shape"][0], d["launch_B"]
    e = dict(d)
    e["shape"] = (B,) + tuple(d["shape"][1:])
    idx = torch.arange(B) % n
    for k in ("x0", "x1", "residual", "pro_a", "pro_b", "res_a", "res_b"):
        if d.get(k) is not None:
            e[k] = d[k][idx]
    return e


# ------------------------------------------------------------------------------------------------------------------------------
# float64 references and tolerances
# ------------------------------------------------------------------------------------------------------------------------------
def conv_reference32(d, kernel, images=None):
    """The output's reference and tolerance for the images `images` (all by default) on `kernel`, with v and its tolerance t32
    for the statistics (the names of the bf16 module's conv_reference, so that its reference() takes this as `core`)."""
    B, C0, C1, Cout, H, W = d["shape"]
    K = d["K"]
    idx = torch.arange(B) if images is None else torch.tensor(sorted(set(images)))
    nb = len(idx)
    x0, wt = d["x0"][idx], d["w"]
    conv = lambda a, w_: F.conv2d(a, w_, padding=K // 2)
    da = None
    if d["pro"]:
        u = x0 * bc(d["pro_a"][idx].double()) + bc(d["pro_b"][idx].double())
        a, da = silu(u), silu_err(u, EPS * u.abs())
    else:
        a = x0 if C1 == 0 else torch.cat([x0, d["x1"][idx]], dim=1)
    bias = d["bias"].double() if d["bias"] is not None else torch.zeros(Cout, dtype=torch.float64)
    v = conv(a, wt) + bias[None, :, None, None]
    amag = a.abs() + (da if da is not None else 0.0)
    P = conv(amag, wt.abs())
    t = chain_terms(kernel, C0 + C1, K) * EPS * (P + bias.abs()[None, :, None, None])
    if da is not None:
        t = t + conv(da, wt.abs())
    if storage_of(kernel) == F16X3:
        wmax = wt.abs().amax(dim=(1, 2, 3))
        ones_w = torch.ones(1, C0 + C1, K, K, dtype=torch.float64)
        t = t + (1 + 2.0 ** -10) * (3 * 2.0 ** -22 * P + 2.0 ** -25 * conv(torch.ones_like(a), wt.abs())) \
              + 2.0 ** -34 * conv(amag, ones_w) * wmax[None, :, None, None]
    ref, tout = v, t
    if d["res"] == "add":
        r = d["residual"][idx]
        ref, tout = v + r, t + EPS * (v.abs() + r.abs())
    elif d["res"] == "tables":
        r = d["residual"][idx]
        u = r * bc(d["res_a"][idx].double()) + bc(d["res_b"][idx].double())
        s = silu(u)
        ref, tout = v + s, t + silu_err(u, EPS * u.abs()) + EPS * (v.abs() + s.abs())
    return dict(images=idx, ref=ref, tol=tout, v=v, t32=t)


def slab_reference(d, core, kernel, tile):
    """(sums, tolerance) (len(images), nslab, G, 2) of every slab the kernel should have written: the sums' formulas on the slab's pixels"""
    B, C0, C1, Cout, H, W = d["shape"]
    G = d["groups"]
    v, t = core["v"], core["t32"]
    nb, cpg, depth = v.shape[0], Cout // G, STAT_DEPTH[kernel]
    smap, nslab = slab_map(kernel, tile, H, W)

    def per_slab(q):                      # (nb, Cout, H, W) -> (nb, nslab, G): summed over the group's channels and the slab's pixels
        pix = q.reshape(nb, G, cpg, H * W).sum(dim=2)
        return torch.zeros(nb, G, nslab, dtype=torch.float64).index_add_(2, smap, pix).permute(0, 2, 1)

    S, Q = per_slab(v), per_slab(v * v)
    tS = per_slab(t) + depth * EPS * per_slab(v.abs())
    tQ = per_slab(2 * v.abs() * t + t * t + EPS * v * v) + depth * EPS * Q
    return torch.stack([S, Q], dim=3), torch.stack([tS, tQ], dim=3)


def slab_ratio(got_slabs, ref, tol):
    """largest error / tolerance over the slabs; a non-finite slab counts as infinite"""
    g_ = got_slabs.double()
    q = (g_ - ref).abs() / tol
    q = torch.where(torch.isfinite(g_), q, torch.full_like(q, float("inf")))
    q = torch.where(g_ == ref, torch.zeros_like(q), q)
    return float(q.max())


def reference32(d, kernel, tile=None, stats=None, images=None, from_output=None, core=None):
    """conv_reference32 plus, with stats = "fused" / "pass", the sums and coefficients (the bf16 module's reference() with this
    kernel's depth) and, fused, the slabs"""
    core = core if core is not None else conv_reference32(d, kernel, images)
    if not stats:
        return dict(core)
    if stats == "pass":
        return reference(d, kernel="gn_stats", core=core, from_output=from_output, depth=STAT_DEPTH["gn_stats"])
    out = reference(d, kernel=kernel, core=core, depth=STAT_DEPTH[kernel])
    out["slabs"], out["slabs_tol"] = slab_reference(d, core, kernel, tile)
    return out


def ratios32(label, got, ref, show=True):
    r = ratios(label, got, ref, show=False)
    if "slabs" in ref:
        r["slabs"] = slab_ratio(got["slabs"][ref["images"]], ref["slabs"], ref["slabs_tol"])
    if show:
        print(f"{label}: largest error / tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# a float32 emulation in the kernels' order: the stand-in kernel of the self-checks below
# ------------------------------------------------------------------------------------------------------------------------------
def split_f16(a):
    """hi, lo of a float32 tensor as float32 tensors of f16 values (round to nearest even, subnormals kept)"""
    hi = a.half().float()
    return hi, (a - hi).half().float()


def pow2_scale(w):
    """(mul, inv) per output channel: the power of two of pow2_channel_scale and its inverse"""
    m = w.abs().amax(dim=(1, 2, 3))
    _, ex = torch.frexp(m.clamp(min=2.0 ** -100))
    k = torch.where(m >= 2.0 ** -100, 10 - ex, torch.zeros_like(ex))
    one = torch.ones_like(m)
    return torch.ldexp(one, k), torch.ldexp(one, -k)


def emulate32(d, kernel, tile=None, stats=False, fault=None):
    """out (and, with stats, slabs, sums, coefficients) as `kernel` would give them.  fault: "drop_slab", "swap_rows",
    "swap_sources", "activate_ring", "next_image_coeffs", "drop_lo", "skip_chunk"."""
    B, C0, C1, Cout, H, W = d["shape"]
    K, G = d["K"], d["groups"]
    nxt = (lambda t: torch.roll(t, -1, dims=0)) if fault == "next_image_coeffs" else (lambda t: t)
    pad = K // 2
    split = storage_of(kernel) == F16X3
    act = silu32 if split else (lambda y: y / (1.0 + torch.exp(-y)))
    if d["pro"]:
        A, Bc = nxt(d["pro_a"]), nxt(d["pro_b"])
        x = f32(d["x0"])
        a = act(fma32(x, bc(A).expand_as(x), bc(Bc).expand_as(x)))
        a = F.pad(a, (pad,) * 4)
        if fault == "activate_ring":
            full = bc(act(Bc)).expand(B, C0, H + 2 * pad, W + 2 * pad).clone()
            full[:, :, pad:pad + H, pad:pad + W] = a[:, :, pad:pad + H, pad:pad + W]
            a = full
    else:
        srcs = [d["x0"]] + ([d["x1"]] if C1 else [])
        if fault == "swap_sources":
            assert C0 == C1
            srcs = srcs[::-1]
        a = F.pad(f32(torch.cat(srcs, dim=1)), (pad,) * 4)
    w = f32(d["w"])
    cin = C0 + C1
    skip = -(-C0 // 32) if fault == "skip_chunk" else -1          # the first chunk that lies in the second source only
    if split:
        mul, inv = pow2_scale(w)
        wh, wl = split_f16(w * mul[:, None, None, None])
        ah, al = split_f16(a)
        if fault == "drop_lo":
            al = torch.zeros_like(al)
        tot = torch.zeros(B, Cout, H, W)
        for c in range(-(-cin // 32)):                             # a chunk's 288-term partial, then the second accumulator set
            if c == skip:
                continue
            s = slice(32 * c, min(cin, 32 * c + 32))
            acc = F.conv2d(al[:, s], wh[:, s]) + F.conv2d(ah[:, s], wl[:, s])
            tot = tot + (acc + F.conv2d(ah[:, s], wh[:, s]))
        v = tot * inv[None, :, None, None]
    else:
        wide = torch.zeros(B, Cout, H, W, dtype=torch.float64)
        for kh in range(K):
            for kw in range(K):
                win = a[:, :, kh:kh + H, kw:kw + W]
                for c in range(-(-cin // 32)):                     # a (tap, chunk) step's 32-term partial, then float64
                    if c == skip:
                        continue
                    s = slice(32 * c, min(cin, 32 * c + 32))
                    wide += torch.einsum("bchw,oc->bohw", win[:, s], w[:, s, kh, kw]).double()
        v = f32(wide)
    if d["bias"] is not None:
        v = v + d["bias"][None, :, None, None]
    o = v
    if d["res"] == "add":
        o = v + f32(d["residual"])
    elif d["res"]:
        A, Bc = nxt(d["res_a"]), nxt(d["res_b"])
        r = f32(d["residual"])
        u = fma32(r, bc(A).expand_as(r), bc(Bc).expand_as(r))
        o = v + u / (1.0 + torch.exp(-u))
    got = dict(out=o.double())
    if not stats:
        return got
    cpg = Cout // G
    smap, nslab = slab_map(kernel, tile, H, W)
    vg = v.reshape(B, G, cpg, H * W)
    pix = torch.stack([vg.sum(dim=2), (vg * vg).sum(dim=2)], dim=3).double()                 # float32 partials, float64 from there
    slabs = f32(torch.zeros(B, G, nslab, 2, dtype=torch.float64).index_add_(2, smap, pix.permute(0, 1, 2, 3))).permute(0, 2, 1, 3).contiguous()
    if fault == "drop_slab":
        slabs[:, nslab // 2] = 0.0
    if fault == "swap_rows":
        assert nslab >= 2
        slabs[:, [0, 1]] = slabs[:, [1, 0]]
    got["slabs"] = slabs.double()
    got["sums"] = slabs.double().sum(dim=1)
    npg = H * W * cpg
    mean = got["sums"][:, :, 0] / npg
    var = (got["sums"][:, :, 1] / npg - mean * mean).clamp(min=0.0)
    mean32, rstd32 = f32(mean).repeat_interleave(cpg, dim=1), f32((var + 1e-5) ** -0.5).repeat_interleave(cpg, dim=1)
    A = rstd32 * d["gamma"][None]
    got.update(coef_a=A.double(), coef_b=(d["beta"][None] - mean32 * A).double())
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# self-checks (CPU)
# ------------------------------------------------------------------------------------------------------------------------------
# every (kernel, tile) of tests/test_gpu_conv_fused_f32.py at its GPU shape (the large batches with two images: the tile is the same)
TILES = [
    ("split_halo", (8, 16, 64), (2, 64, 64, 64, 16, 32)),
    ("split_halo", (4, 32, 64), (2, 64, 64, 64, 12, 32)),
    ("split_ws", (8, 16, 128), (2, 64, 64, 128, 16, 16)),
    ("split_w512", (16, 16, 128), (2, 64, 64, 128, 16, 16)),
    ("split_p64", (16, 16, 64), (2, 64, 64, 64, 32, 32)),
    ("split_igemm", (128, 64), (3, 72, 48, 64, 16, 8)),
    ("halo", (8, 32, 64), (2, 64, 64, 64, 16, 32)),
    ("halo", (8, 16, 64), (2, 64, 64, 64, 16, 16)),
    ("halo", (4, 32, 128), (2, 64, 64, 128, 12, 32)),
    ("halo", (8, 16, 128), (2, 64, 64, 128, 16, 16)),
    ("igemm", (128, 64), (3, 72, 48, 64, 16, 8)),
]
TILE_IDS = [f"{k} {'x'.join(map(str, t))}" for k, t, _ in TILES]
HALO_TILES = [t for t in TILES if "igemm" not in t[0]]
HALO_IDS = [f"{k} {'x'.join(map(str, t))}" for k, t, _ in HALO_TILES]


def single(shape):
    B, C0, C1, Cout, H, W = shape
    return (B, C0, 0, Cout, H, W)


def check32(d, kernel, tile, stats=False, fault=None, label=""):
    got = emulate32(d, kernel, tile, stats=stats, fault=fault)
    ref = reference32(d, kernel, tile, stats="fused" if stats else None)
    return ratios32(f"{label} [{kernel} {'x'.join(map(str, tile))}]" + (f" fault={fault}" if fault else ""), got, ref)


@pytest.mark.parametrize("kernel,tile,shape", TILES, ids=TILE_IDS)
def test_faithful_emulation_passes(kernel, tile, shape):
    for fam in ("normal", "amplitude", "tiny", "zero_x0", "zero_x1"):
        sh = (6,) + shape[1:] if fam == "amplitude" else shape
        r = check32(make_case32(sh, family=fam, seed=11), kernel, tile, stats=True, label=f"two sources, {fam}")
        assert max(r.values()) < 1.0, (fam, r)
    r = check32(make_case32(shape, bias=False, seed=12), kernel, tile, stats=True, label="no bias")
    assert max(r.values()) < 1.0, r
    if "igemm" not in kernel:
        for fam in ("normal", "border", "amplitude", "tiny"):
            r = check32(make_case32(single(shape), pro="tables", family=fam, seed=13), kernel, tile, stats=True, label=f"table prologue, {fam}")
            assert max(r.values()) < 1.0, (fam, r)
    # a subset of the images is the same reference
    d = make_case32(shape, seed=11)
    sub, full = conv_reference32(d, kernel, images=[0, shape[0] - 1]), conv_reference32(d, kernel)
    last = shape[0] - 1
    assert torch.allclose(sub["ref"], full["ref"][[0, last]], rtol=1e-12, atol=0) and torch.allclose(sub["tol"], full["tol"][[0, last]], rtol=1e-12, atol=0)


@pytest.mark.parametrize("kernel", ("split_igemm", "igemm"))
@pytest.mark.parametrize("res", (None, "add", "tables"))
def test_faithful_1x1_emulation_passes(kernel, res):
    for shape in ((8, 64, 64, 64, 6, 6), (3, 128, 0, 64, 12, 12), (1, 384, 384, 512, 8, 8)):
        for fam in ("normal", "amplitude", "tiny"):
            d = make_case32(shape, K=1, res=res, family=fam, seed=14)
            r = check32(d, kernel, (128, 64), label=f"1x1 {shape} residual={res}, {fam}")
            assert r["out"] < 1.0, (shape, fam, r)
    if res == "tables":
        d = make_case32((3, 128, 0, 64, 12, 12), K=1, res=res, seed=15)
        assert check32(d, kernel, (128, 64), fault="next_image_coeffs", label="1x1 tables")["out"] > 1.0


@pytest.mark.parametrize("kernel,tile,shape", TILES, ids=TILE_IDS)
def test_a_dropped_slab_fails(kernel, tile, shape):
    d = make_case32(shape, seed=5)
    bad = check32(d, kernel, tile, stats=True, fault="drop_slab")
    assert bad["out"] < 1.0 and bad["sums"] > 1.0 and bad["slabs"] > 1.0 and bad["coef_a"] > 1.0, bad


@pytest.mark.parametrize("kernel,tile,shape", HALO_TILES, ids=HALO_IDS)
def test_swapped_wave_row_slabs_fail_the_slab_comparison_only(kernel, tile, shape):
    # slabs 0 and 1: the two wave rows of a tile (ws, w512, p64), the first two tiles of the others.  Same sums, other places.
    d = make_case32(shape, seed=5)
    bad = check32(d, kernel, tile, stats=True, fault="swap_rows")
    assert bad["slabs"] > 1.0, bad
    assert max(bad["out"], bad["sums"], bad["coef_a"], bad["coef_b"]) < 1.0, bad


@pytest.mark.parametrize("kernel,tile,shape", HALO_TILES, ids=HALO_IDS)
def test_swapped_sources_fail(kernel, tile, shape):
    for fam in ("normal", "zero_x0", "zero_x1"):
        assert check32(make_case32(shape, family=fam, seed=6), kernel, tile, fault="swap_sources", label=fam)["out"] > 1.0


@pytest.mark.parametrize("kernel,tile,shape", HALO_TILES, ids=HALO_IDS)
def test_an_activated_padding_ring_fails(kernel, tile, shape):
    for fam in ("normal", "border"):
        d = make_case32(single(shape), pro="tables", family=fam, seed=7)
        got, ref = emulate32(d, kernel, tile, fault="activate_ring"), reference32(d, kernel, tile)
        assert ratios32(f"padding ring activated, {fam} [{kernel}]", got, ref)["out"] > 1.0
        inner = ((got["out"] - ref["ref"]).abs() / ref["tol"])[:, :, 1:-1, 1:-1]
        assert float(inner.max()) < 1.0                            # only the edge pixels notice


@pytest.mark.parametrize("kernel,tile,shape", HALO_TILES, ids=HALO_IDS)
def test_the_next_images_coefficients_fail(kernel, tile, shape):
    d = make_case32(single(shape), pro="tables", seed=8)
    assert check32(d, kernel, tile, fault="next_image_coeffs")["out"] > 1.0


@pytest.mark.parametrize("kernel,tile,shape", [t for t in TILES if t[0].startswith("split")], ids=[i for i in TILE_IDS if i.startswith("split")])
def test_a_dropped_lo_half_fails(kernel, tile, shape):
    d = make_case32(shape, seed=9)
    r = check32(d, kernel, tile, fault="drop_lo")
    assert r["out"] > 1.0, r
    # a bf16-grade tolerance (the bf16 module's: n + 1 accumulations and half a bf16 ulp of the output) would pass it
    got, ref = emulate32(d, kernel, tile, fault="drop_lo"), conv_reference32(d, kernel)
    n = (shape[1] + shape[2]) * 9
    coarse = float(((got["out"] - ref["ref"]).abs() / (2.0 ** -9 * ref["ref"].abs() + ref["tol"] * (n + 1) / chain_terms(kernel, n // 9, 3))).max())
    print(f"lo half dropped [{kernel}]: against a bf16-grade tolerance {coarse:.3g}")
    assert coarse < 1.0
    for one in ((8, 64, 64, 64, 6, 6), (1, 384, 384, 512, 8, 8)):
        if kernel == "split_igemm":
            assert check32(make_case32(one, K=1, seed=9), kernel, tile, fault="drop_lo", label=f"1x1 {one}")["out"] > 1.0


@pytest.mark.parametrize("kernel,tile,shape", TILES, ids=TILE_IDS)
def test_a_skipped_chunk_of_the_second_source_fails(kernel, tile, shape):
    assert check32(make_case32(shape, seed=10), kernel, tile, fault="skip_chunk")["out"] > 1.0


def test_chain_terms_and_the_conv_level_bound():
    assert chain_terms("split_halo", 64, 3) == 288 + 2 + 1 and chain_terms("split_ws", 192, 3) == 288 + 6 + 1
    assert chain_terms("split_igemm", 120, 3) == 256 + 5 + 1 and chain_terms("split_igemm", 768, 1) == 256 + 3 + 1
    assert chain_terms("halo", 576, 3) == 34 and chain_terms("igemm", 768, 1) == 34
    # K = 576 (64 channels, 3x3), in units of e P: the split alone stays inside the conv-level bound 2^-19 of tests/test_gpu_f16x3.py;
    # with the worst-case chain it is ten times looser (the docstring says why)
    split = 3 * 2.0 ** -22 * (1 + 2.0 ** -10) / EPS
    assert split < 2.0 ** -19 / EPS == 32.0
    assert math.isclose(split + chain_terms("split_halo", 64, 3), 303.01, abs_tol=0.01)


def test_slab_maps_partition_the_image():
    for kernel, tile, shape in TILES:
        H, W = shape[4], shape[5]
        m, n = slab_map(kernel, tile, H, W)
        counts = torch.bincount(m, minlength=n)
        assert len(counts) == n and int(counts.min()) == int(counts.max()) == H * W // n, (kernel, tile)
    m, _ = slab_map("split_ws", (8, 16, 128), 16, 32)
    assert m.reshape(16, 32)[4, 0] == 1 and m.reshape(16, 32)[0, 16] == 2 and m.reshape(16, 32)[8, 0] == 4
    m, _ = slab_map("split_p64", (16, 16, 64), 32, 32)
    assert m.reshape(32, 32)[4, 0] == 1 and m.reshape(32, 32)[0, 16] == 4 and m.reshape(32, 32)[16, 0] == 8


# ------------------------------------------------------------------------------------------------------------------------------
# the GPU module's expectations against the library's own selection (prg_debug_conv_choice: host only), at 256 CUs
# ------------------------------------------------------------------------------------------------------------------------------
def selection(storage, shape, K, groups, stats, pro=False, residual=False, res_a=False, num_cus=256, p64=256, w512=1):
    """((family, th, tw, bm, bn), nsplit) of choose_conv for the launch the hook makes"""
    from pointreggpt_amd import _lib
    B, C0, C1, Cout, H, W = shape
    present = 1 | (512 if storage == F16X3 else 0) | (8 if pro else 0) | (16 if stats else 0) | (2 if residual else 0) | (4 if res_a else 0)
    q = [_lib.PRG_F16X3 if storage == F16X3 else _lib.PRG_F32, B, H, W, C0, C1, 0, K, K, 1, K // 2, H, W, Cout, -(-Cout // 64) * 64,
         -(-(C0 + C1) // 16), present, groups, 0, 0, 0, 0, 0, num_cus, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, p64, w512]
    out, scale = (C.c_int32 * 32)(), C.c_float()
    assert len(q) == 36
    _lib.check(_lib.load().prg_debug_conv_choice((C.c_int32 * 36)(*q), None, out, C.byref(scale)), "prg_debug_conv_choice")
    assert not pro or out[16] == 1, (shape, "conv_supports_prologue declines: the hook would reject the prologue")
    return (_lib.CONV_FAMILIES[out[0]], out[1], out[2], out[3], out[4]), out[12]


def test_the_gpu_modules_expectations_match_the_selection():
    import test_gpu_conv_fused_f32 as g
    n = 0
    for name, (shape, groups, kernel, tile, distinct, modes) in g.cases3(256).items():
        for stats in modes:
            choice, flags = g.expected(kernel, tile, shape, groups, stats)
            assert selection(storage_of(kernel), shape, 3, groups, stats) == (choice, flags[0]), (name, stats)
            n += 1
    for name, (shape, kernel, tile, distinct) in g.cases_pro(256).items():
        for stats in (0, 1):
            choice, flags = g.expected(kernel, tile, shape, 8, stats)
            assert selection(storage_of(kernel), shape, 3, 8, stats, pro=True) == (choice, flags[0]), (name, stats)
            n += 1
    for name, (shape, tile) in g.CASES1.items():
        for kernel in ("split_igemm", "igemm"):
            for res in (None, "add", "tables"):
                choice, _ = g.expected(kernel, tile, shape, 8, 0)
                assert selection(storage_of(kernel), shape, 1, 8, 0, residual=bool(res), res_a=res == "tables")[0] == choice, (name, kernel, res)
                n += 1
    for name, (shape, K, kernel, tile, exact) in g.ZERO.items():
        assert selection(storage_of(kernel), shape, K, 8, 0)[0] == g.expected(kernel, tile, shape, 8, 0)[0], name
        n += 1
    for name, batch in g.AMP_CASES.items():
        shape, groups, kernel, tile, distinct, modes = g.cases3(256)[name]
        if batch:
            shape = (batch,) + shape[1:]
        for stats in modes:
            choice, flags = g.expected(kernel, tile, shape, groups, stats)
            assert selection(storage_of(kernel), shape, 3, groups, stats) == (choice, flags[0]), (name, stats)
            n += 1
    for name, (shape, kernel, tile) in g.STRADDLE.items():                # groups that do not divide the channel tile: never fused
        assert selection(storage_of(kernel), shape, 3, 8, 1) == (g.expected(kernel, tile, shape, 8, 0)[0], 0), name
        assert g.expected(kernel, tile, shape, 8, 1)[1] == (0, 0, 1)
        n += 1
    for name, shape, kernel, tile, pro in g.FORCED:
        for stats in (0, 1):
            choice, flags = g.expected(kernel, tile, shape, 8, stats)
            assert selection(F16X3, shape, 3, 8, stats, pro=bool(pro), p64=1, w512=2) == (choice, flags[0]), (name, stats)
            n += 1
    # tile_fuse in bf16 (the halo kernel behind conv_ws's refusal of three channel tiles) and on the gather kernels' 64-channel tile
    for dtype, split in ((1, 0), (0, 0), (3, 512)):
        for shape in ((2, 64, 0, 192, 16, 32), (2, 64, 0, 192, 16, 8)):
            B, C0, C1, Cout, H, W = shape
            q = [dtype, B, H, W, C0, C1, 0, 3, 3, 1, 1, H, W, Cout, 192, 4, 1 | 16 | split, 8, 0, 0, 0, 0, 0, 256, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 256, 1]
            from pointreggpt_amd import _lib
            out, scale = (C.c_int32 * 32)(), C.c_float()
            _lib.check(_lib.load().prg_debug_conv_choice((C.c_int32 * 36)(*q), None, out, C.byref(scale)), "prg_debug_conv_choice")
            assert out[0] > 0 and out[11] == 0 and out[12] == 0, (dtype, shape, list(out[:14]))
            n += 1
    print(f"{n} expectations of tests/test_gpu_conv_fused_f32.py agree with choose_conv at 256 CUs")
