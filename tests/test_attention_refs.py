"""What the attention tests stand on, checked without a GPU: the float64 references of the attention cores, the channel LayerNorm
and the Residual(PreNorm(LinearAttention)) block, the input families, the tolerances computed from the inputs, and the emulation of
the fused blocks at the kernels' precision.  tests/test_gpu_attention.py imports all of it and compares the HIP kernels with it.

Input families of the cores (qkv is the to_qkv output, (B, 384, N): q | k | v, each 4 heads x 32, head-major):
  F1 peaked    q, k ~ 2.2 N(0,1), v ~ N(0,1): logit std ~4.9, median row-max probability ~0.5.
  F2 pointer   k_j ~ N(0,1) scaled to norm sqrt(32), q_i = 6 k_pi(i) for a random permutation pi, v_j[e] = ((j (e+1)) mod 17 - 8) / 4:
               every query points at one key (top probability > 0.9, asserted) and v names the key.  Without the fixed norm a
               short k_pi(i) (chi^2 with 32 degrees: |k|^2 down to ~10 among 10^4 keys) has its own logit 6 |k|^2 / sqrt(32) ~ 11
               below the largest stranger's, and the asserted 0.9 cannot hold at N = 1024.  For the linear core four columns of
               every head get one pixel with k + 12: the softmax over pixels points as well.
  F3 shifted   F1 with dimension 0 of every q = 8 and of every k = +50 (image 0), -50 (image 1): +-70.7 on every logit of a row,
               the softmax is unchanged, a kernel without the row maximum overflows or underflows.  Image 2 is stepped: -50 for
               the keys before max(N / 2, 32), +50 from there on — the maximum has to be taken over ALL keys (see the power check).
  F4           q, k, v ~ N(0,1) with one NaN in v, one NaN in k or one +Inf in v.  The base is soft on purpose: Inf times a
               probability is Inf only while the probability is not zero in the kernel's format, and the f16 halves of the split
               kernel underflow at 2^-25; logits of std 1 keep every probability above e^-12.

Tolerances follow the derivations in the functions' comments; none is fitted to an observed error.
"""
import math

import pytest
import torch

from oracle import unet as OU

HEADS, DH, HID = 4, 32, 128
SCALE = DH ** -0.5
LOG2E_F32 = 1.4426950408889634

FULL_GENERIC_N = (1, 36, 127, 128, 129, 257, 400)
FULL_MFMA_N = (64, 128, 256, 512, 1024)
FULL_SPLIT_N = (128, 256, 512, 1024)
LINEAR_N = (1, 63, 512, 513, 1600, 4097)
CAP_F32, CAP_BF16 = 2.0 ** -12, 2.0 ** -6         # of V = max |v|, on F1 and F2

LN_C_F32 = (8, 16, 24, 64, 128, 256, 512)
LN_C_BF16 = (8, 16, 24, 64, 256, 512)
LN_M = (1, 63, 1000)

BLOCK_N_BF16 = (16, 100, 576, 1088, 1600)
BLOCK_N_SPLIT = (64, 576, 1088, 1600)
STATIC_LIMIT = 40.0 * LOG2E_F32                   # unet_weights.hip: the largest static softmax bound, log2 units
EMU_CAP_MAX, EMU_CAP_MEAN = 0.05, 0.006


def bf16(t):
    """round to bf16 (nearest even), back in the tensor's own dtype"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def heads(qkv):
    B, _, N = qkv.shape
    return tuple(t.reshape(B, HEADS, DH, N) for t in qkv.chunk(3, dim=1))


def _finite(t):
    return torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)


def bf16_half_ulp(t):
    """The largest error of storing a value of magnitude <= t as bf16 (8 significant bits): half an ulp of t's binade,
    2^(floor(log2 t) - 8) — between 2^-9 t (t just below a power of two) and 2^-8 t (t a power of two).  A flat 2^-9 t is only the
    lower end: a stored 2.03 may be off by 2^-8 = 1.9e-3 t."""
    t = t.abs().double()
    return torch.where(t > 0, torch.exp2(torch.floor(torch.log2(t.clamp(min=1e-300))) - 8), torch.zeros_like(t))


# ------------------------------------------------------------------------------------------------------------------------
# references (float64), with the known defects of the power check
# ------------------------------------------------------------------------------------------------------------------------
def _swap_pairs(n):
    idx = torch.arange(n) ^ 1
    idx[idx >= n] = n - 1
    return idx


def ref_full(qkv, defect=None):
    """oracle.unet.full_attention without its convs: softmax(q k^T / sqrt(32)) v, (B, 384, N) -> (B, 128, N)"""
    q, k, v = heads(qkv.double())
    B, N = qkv.shape[0], qkv.shape[2]
    sim = torch.einsum("bhdi,bhdj->bhij", q * SCALE, k)
    if defect == "drop_last":
        sim, v = sim[..., :-1], v[..., :-1]
    if defect == "partial_max":          # the row maximum over the first 32 keys only, exp in float32
        p = torch.exp((sim - sim[..., :32].amax(-1, keepdim=True)).float()).double()
        p = p / p.sum(-1, keepdim=True)
    else:
        p = sim.softmax(dim=-1)
    if defect == "swap_v":
        v = v[..., _swap_pairs(N)]
    return torch.einsum("bhij,bhdj->bhid", p, v).permute(0, 1, 3, 2).reshape(B, HID, N)


def ref_linear(qkv, defect=None):
    """oracle.unet.linear_attention without its convs and LayerNorm"""
    q, k, v = heads(qkv.double())
    B, N = qkv.shape[0], qkv.shape[2]
    q = q.softmax(dim=-2) * SCALE
    if defect == "drop_last":
        k = torch.cat([k[..., :-1].softmax(dim=-1), torch.zeros_like(k[..., -1:])], dim=-1)
    else:
        k = k.softmax(dim=-1)
    if defect == "swap_v":
        v = v[..., _swap_pairs(N)]
    ctx = torch.einsum("bhdn,bhen->bhde", k, v / N)
    return torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, HID, N)


def ref_layernorm(x, g, residual=None):
    """oracle.unet.channel_layernorm on pixel-major rows (M, C), float64, plus the residual"""
    y = OU.channel_layernorm(x.double().t()[None], g.double()[None, :, None])[0].t()
    return y if residual is None else y + residual.double()


def ref_block(x, norm_g, w_qkv, w_out, b_out, out_g):
    """oracle.unet.prenorm_residual(..., linear_attention) in float64 on (B, C, N)"""
    B, C, N = x.shape
    p = {"a.fn.norm.g": norm_g.double().reshape(1, C, 1, 1), "a.fn.fn.to_qkv.weight": w_qkv.double().reshape(3 * HID, C, 1, 1),
         "a.fn.fn.to_out.0.weight": w_out.double().reshape(C, HID, 1, 1), "a.fn.fn.to_out.0.bias": b_out.double(),
         "a.fn.fn.to_out.1.g": out_g.double().reshape(1, C, 1, 1)}
    return OU.prenorm_residual(p, "a", x.double().reshape(B, C, N, 1), OU.linear_attention).reshape(B, C, N)


# ------------------------------------------------------------------------------------------------------------------------
# input families of the cores
# ------------------------------------------------------------------------------------------------------------------------
POINTED_COLUMNS = (0, 5, 17, 31)
F4_POS = dict(h=2, e=5, d=7)


def pointer_perm(N, g):
    return torch.randperm(N, generator=g)


def make_qkv(family, B, N, seed, linear=False):
    g = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn((B, HEADS, DH, N), generator=g, dtype=torch.float64)        # noqa: E731
    if family in ("F1", "F3"):
        q, k, v = 2.2 * rn(), 2.2 * rn(), rn()
        if family == "F3":
            q[:, :, 0, :] = 8.0
            k[0, :, 0, :] = 50.0
            if B > 1:
                k[1, :, 0, :] = -50.0
            if B > 2:
                step = max(N // 2, min(32, N - 1))
                k[2, :, 0, :step] = -50.0
                k[2, :, 0, step:] = 50.0
    elif family == "F2":
        k = rn()
        k = k * (math.sqrt(DH) / k.norm(dim=2, keepdim=True))
        q = 6.0 * k[..., pointer_perm(N, g)]
        j, e = torch.arange(N, dtype=torch.float64)[None, :], torch.arange(DH, dtype=torch.float64)[:, None]
        v = (((j * (e + 1)) % 17 - 8) / 4).expand(B, HEADS, DH, N).clone()
        if linear:
            for h in range(HEADS):
                for d in POINTED_COLUMNS:
                    k[:, h, d, int(torch.randint(N, (1,), generator=g))] += 12.0
    elif family.startswith("F4"):
        q, k, v = rn(), rn(), rn()
    else:
        raise ValueError(family)
    qkv = torch.cat([t.reshape(B, HID, N) for t in (q, k, v)], dim=1).float()
    if family.startswith("F4"):
        b0, j, P = B - 1, N // 2, F4_POS
        if family == "F4_nan_v":
            qkv[b0, 2 * HID + P["h"] * DH + P["e"], j] = float("nan")
        elif family == "F4_nan_k":
            qkv[b0, HID + P["h"] * DH + P["d"], j] = float("nan")
        elif family == "F4_inf_v":
            qkv[b0, 2 * HID + P["h"] * DH + P["e"], j] = float("inf")
        else:
            raise ValueError(family)
    return qkv


# ------------------------------------------------------------------------------------------------------------------------
# tolerances of the cores: one number per (image, head), shape (B, 4, 1, 1) against the output as (B, 4, 32, N)
# ------------------------------------------------------------------------------------------------------------------------
def full_stats(qkv):
    q, k, v = heads(_finite(qkv.double()))
    V = v.abs().amax(dim=(2, 3))
    S_abs = torch.einsum("bhdi,bhdj->bhij", q.abs() * SCALE, k.abs()).amax(dim=(2, 3))
    sim = torch.einsum("bhdi,bhdj->bhij", q * SCALE, k)
    R = (sim.amax(-1) - sim.amin(-1)).amax(-1)
    return V, S_abs, R


def full_tol(qkv, variant):
    """If every logit is off by at most d, each probability moves by a factor within e^{+-2d}: |out error| <= (e^{2d} - 1) V.
    f32   float32 logits (32 fmafs and the scale: 34 roundings of at most S_abs each) and expf: d = 34 2^-24 S_abs + 2^-22;
          float64 sums; the division and the store: 2^-23 V.
    bf16  the same kernel on bf16 storage: float32 sums over N keys (N 2^-24 V) and the bf16 store of a value <= V: half an ulp of
          V's binade (bf16_half_ulp; a flat 2^-9 V holds only for V just below a power of two).
    mfma  d + 2^-24 1.45 R for the scale applied to the accumulated logit (R = largest range of a row's logits, log2 e = 1.45);
          p rounded to bf16 in the numerator only (2^-9 V), the store (bf16_half_ulp(V)); twice the sum for the hardware exp2 and
          the accumulation order.
    split the per-product bound of the split-f16 contractions (test_gpu_f16x3.py): d = 2^-19 S_abs + 2^-22, and
          (2^-19 + 2^-22) V for the P V contraction."""
    N = qkv.shape[2]
    V, S, R = full_stats(qkv)
    d = 34 * 2.0 ** -24 * S + 2.0 ** -22
    if variant == "f32":
        t = torch.expm1(2 * d) * V + 2.0 ** -23 * V
    elif variant == "bf16":
        t = torch.expm1(2 * d) * V + N * 2.0 ** -24 * V + bf16_half_ulp(V)
    elif variant == "mfma":
        t = 2 * (torch.expm1(2 * (d + 2.0 ** -24 * 1.45 * R)) * V + 2.0 ** -9 * V + bf16_half_ulp(V))
    elif variant == "split":
        t = torch.expm1(2 * (2.0 ** -19 * S + 2.0 ** -22)) * V + (2.0 ** -19 + 2.0 ** -22) * V
    else:
        raise ValueError(variant)
    return t[:, :, None, None], V[:, :, None, None]


def linear_tol(qkv, variant):
    """Both softmaxes move by e^{+-2d} with d = 2^-22 + 2^-24 R (expf, and the subtraction of the maximum at the range R of the
    column of k / the row of q); 40 2^-24 for la_fin and the 32 fmafs; bf16: (N + 40) 2^-24 for the float32 sums over the pixels.
    All relative to the largest output there can be: the reference divides v by N, so |out| <= sum_d |ctx[d][e]| q'[d] <=
    (V / N) 32^-1/2.  bf16: plus the store of a value of at most that size, bf16_half_ulp of it."""
    N = qkv.shape[2]
    q, k, v = heads(_finite(qkv.double()))
    V = v.abs().amax(dim=(2, 3))
    Rk = (k.amax(-1) - k.amin(-1)).amax(-1)
    Rq = (q.amax(2) - q.amin(2)).amax(-1)
    rel = torch.expm1(2 * (2.0 ** -22 + 2.0 ** -24 * Rk) + 2 * (2.0 ** -22 + 2.0 ** -24 * Rq)) + 40 * 2.0 ** -24
    big = SCALE * V / N
    if variant == "bf16":
        t = (rel + (N + 40) * 2.0 ** -24) * big + bf16_half_ulp(big)
    elif variant == "f32":
        t = rel * big
    else:
        raise ValueError(variant)
    return t[:, :, None, None], V[:, :, None, None]


def layernorm_tol(x, g, ref, dtype, residual):
    """per element 16 2^-24 (max_c |x| / sigma) |g_c|, sigma = sqrt(var + 1e-5): the float32 mean and deviations carry errors of a
    few ulp of max |x|, amplified by 1 / sigma.  bf16: the store, half an ulp of the stored value (bf16_half_ulp(ref), up to
    2^-8 |ref|).  With a residual in float32 the sum is rounded once more: 2^-24 |ref|."""
    x = x.double()
    sigma = (x.var(dim=1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    t = 16 * 2.0 ** -24 * (x.abs().amax(dim=1, keepdim=True) / sigma) * g.double().abs()[None, :]
    if dtype == "bf16":
        t = t + bf16_half_ulp(_finite(ref))
    elif residual is not None:
        t = t + 2.0 ** -24 * ref.abs()
    return t


def exceeds(out, ref, tol):
    """True where `out` is not an acceptable answer: non-finite where the reference is finite, or further than tol"""
    B, _, N = ref.shape
    o, r = out.reshape(B, HEADS, DH, N), ref.reshape(B, HEADS, DH, N)
    return (~torch.isfinite(o) & torch.isfinite(r)) | ((o - r).abs() > tol)


# ------------------------------------------------------------------------------------------------------------------------
# the fused blocks: families and the emulation at the kernels' precision
# ------------------------------------------------------------------------------------------------------------------------
def fold_qkv(w_qkv, norm_g):
    """to_qkv with the PreNorm gain folded in, q and k rows times log2 e, in float32 in the packer's order of operations"""
    w = w_qkv.float() * norm_g.float()[None, :]
    w[:2 * HID] = w[:2 * HID] * torch.tensor(LOG2E_F32, dtype=torch.float32)
    return w


def static_bounds(w_qkv, norm_g):
    """unet_weights.hip: 1.02 ||w_d|| sqrt(C) of the bf16 q and k rows, log2 units"""
    C = w_qkv.shape[1]
    w = bf16(fold_qkv(w_qkv, norm_g)).double()[:2 * HID]
    return 1.02 * (w.pow(2).sum(dim=1) * C).sqrt()


def block_weights(C, seed, family="R"):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)        # noqa: E731
    norm_g, out_g = 1 + 0.2 * rn(C), 1 + 0.2 * rn(C)
    w_qkv = rn(3 * HID, C) / math.sqrt(C)
    w_qkv[:2 * HID] *= 3.0
    w_out, b_out = rn(C, HID) / math.sqrt(HID), 0.1 * rn(C)
    if family == "E":       # every q / k row at a static bound of 56 log2 units
        w_qkv[:2 * HID] *= (56.0 / static_bounds(w_qkv, norm_g)).float()[:, None]
    return dict(norm_g=norm_g, w_qkv=w_qkv, w_out=w_out, b_out=b_out, out_g=out_g)


def block_x(W, B, N, seed, family="R"):
    g = torch.Generator().manual_seed(seed)
    C = W["w_qkv"].shape[1]
    if family == "R":
        return 1.5 * torch.randn((B, C, N), generator=g) + 0.3
    # E: pixels along -+ the folded k row of largest norm, so that LayerNorm(x) is aligned with it
    wk = (W["w_qkv"] * W["norm_g"][None, :])[HID:2 * HID]
    w = wk[wk.norm(dim=1).argmax()]
    sign = torch.where(torch.arange(N) % 2 == 0, -2.0, 2.0)
    return sign[None, None, :] * (w - w.mean())[None, :, None] + 0.05 * torch.randn((B, C, N), generator=g)


def _ln64(x, dim):
    return (x - x.mean(dim, keepdim=True)) * (x.var(dim=dim, unbiased=False, keepdim=True) + 1e-5).rsqrt()


def emulate_block(x, norm_g, w_qkv, w_out, b_out, out_g, mode):
    """The block evaluated in float64 with roundings where the kernels' headers say they round.
    mode "bf16" (attn_fused.hip): bf16 at LayerNorm(x), the folded weights, p = exp2(k - max), v, ctx, the normalised q', the
      attention output o, w_out, the normalised y, the stored sum; sums exact (the kernels': float32).
    mode "f16x3" (attn_split.hip): every contraction on operands cut to hi + lo f16 halves (22 bits; the dropped lo x lo product is
      not modelled), everything between the contractions in float32."""
    B, C, N = x.shape
    if mode == "bf16":
        r = bf16
        xn = r(_ln64(x.double(), 1))
        qkv = torch.einsum("oc,bcn->bon", r(fold_qkv(w_qkv, norm_g)).double(), xn)
        q, k, v = heads(qkv)
        p = r(torch.exp2(k - k.amax(-1, keepdim=True)))
        ctx = r(torch.einsum("bhdn,bhen->bhde", p, r(v)) / torch.exp2(k - k.amax(-1, keepdim=True)).sum(-1)[..., None] * (SCALE / N))
        qs = r((q * math.log(2.0)).softmax(dim=2))
        o = r(torch.einsum("bhde,bhdn->bhen", ctx, qs).reshape(B, HID, N))
        y = torch.einsum("ck,bkn->bcn", r(w_out.float()).double(), o) + b_out.double()[None, :, None]
        return r(r(_ln64(y, 1) * out_g.double()[None, :, None]) + x.double())
    if mode != "f16x3":
        raise ValueError(mode)
    f32 = torch.float32

    def cut(t):                                     # a float32 value as the sum of its two f16 halves
        t = t.to(f32)
        hi = t.half().to(f32)
        return (hi + (t - hi).half().to(f32)).double()

    xf = x.to(f32)
    xn = (xf - xf.mean(1, keepdim=True)) * (xf.var(dim=1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    q, k, v = heads(torch.einsum("oc,bcn->bon", cut(fold_qkv(w_qkv, norm_g)), cut(xn)).to(f32))
    p = torch.exp2(k - k.amax(-1, keepdim=True))
    ctx = torch.einsum("bhdn,bhen->bhde", cut(p), cut(v)).to(f32) / p.double().sum(-1).to(f32)[..., None] * (SCALE / N)
    qs = torch.exp2(q - q.amax(2, keepdim=True))
    qs = qs / qs.sum(2, keepdim=True)
    o = torch.einsum("bhde,bhdn->bhen", cut(ctx), cut(qs)).to(f32).reshape(B, HID, N)
    y = torch.einsum("ck,bkn->bcn", cut(w_out), cut(o)).to(f32) + b_out.to(f32)[None, :, None]
    yn = (y - y.mean(1, keepdim=True)) * (y.var(dim=1, unbiased=False, keepdim=True) + 1e-5).rsqrt() * out_g.to(f32)[None, :, None]
    return (yn + xf).double()


def block_case(C, B, N, family, mode):
    """weights, the x the kernel receives, the float64 reference and the emulation's error against it"""
    W = block_weights(C, 1000 + C, family)
    x = block_x(W, B, N, 7 * C + 13 * B + N, family)
    if mode == "bf16":
        x = bf16(x)
    ref = ref_block(x, **W)
    err = (emulate_block(x, mode=mode, **W) - ref).abs()
    return W, x, ref, float(err.max()), float(err.mean())


# ------------------------------------------------------------------------------------------------------------------------
# CPU checks
# ------------------------------------------------------------------------------------------------------------------------
def test_references_are_the_oracles_functions():
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn((2, 3 * HID, 6, 5), generator=g, dtype=torch.float64)
    eye = lambda n: torch.eye(n, dtype=torch.float64).reshape(n, n, 1, 1)        # noqa: E731
    p = {"a.to_qkv.weight": eye(3 * HID), "a.to_out.weight": eye(HID), "a.to_out.bias": torch.zeros(HID, dtype=torch.float64),
         "a.to_out.0.weight": eye(HID), "a.to_out.0.bias": torch.zeros(HID, dtype=torch.float64),
         "a.to_out.1.g": torch.ones((1, HID, 1, 1), dtype=torch.float64)}
    flat = qkv.reshape(2, 3 * HID, 30)
    assert torch.allclose(ref_full(flat).reshape(2, HID, 6, 5), OU.full_attention(p, "a", qkv), rtol=0, atol=1e-13)
    lin = OU.channel_layernorm(ref_linear(flat).reshape(2, HID, 6, 5), p["a.to_out.1.g"])
    assert torch.allclose(lin, OU.linear_attention(p, "a", qkv), rtol=0, atol=1e-11)
    x, gain, res = torch.randn((7, 24), generator=g), torch.randn(24, generator=g), torch.randn((7, 24), generator=g)
    want = torch.nn.functional.layer_norm(x.double(), (24,), eps=1e-5) * gain.double() + res.double()
    assert torch.allclose(ref_layernorm(x, gain, res), want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("N", sorted(set(FULL_GENERIC_N + FULL_MFMA_N + FULL_SPLIT_N)))
def test_bottleneck_families_bounds_and_power(N):
    """The families' own conditions, every bound finite and under its cap, and the power of the comparison: a reference with a
    known defect must be rejected, with the tolerances the GPU test uses, on F1 or F2 —
      * V's keys swapped pairwise and the last key dropped: at every N >= 2 (N = 1 has no second key);
      * the row maximum over the first 32 keys with exp in float32: NOT on F1 / F2, at any N.  The softmax does not depend on the
        shift, the defect only shows once exp overflows (a later logit 88.7 above those 32), and F1's rows span ~30, F2's < 54.
        F3's stepped image is there for it: its second half lies 141 above its first, and the defect must be rejected there at
        every N > 32 (up to 32 keys it is no defect)."""
    B = 3
    variants = [v for v, ns in (("f32", FULL_GENERIC_N), ("bf16", FULL_GENERIC_N), ("mfma", FULL_MFMA_N), ("split", FULL_SPLIT_N)) if N in ns]
    caught = {d: False for d in ("swap_v", "drop_last")}
    for fam in ("F1", "F2", "F3"):
        qkv = make_qkv(fam, B, N, 100 + N)
        ref = ref_full(qkv)
        assert torch.isfinite(ref).all()
        if fam == "F2":
            q, k, _ = heads(qkv.double())
            top = torch.einsum("bhdi,bhdj->bhij", q * SCALE, k).softmax(-1).amax(-1)
            assert float(top.min()) > 0.9, float(top.min())
            pi = torch.einsum("bhdi,bhdj->bhij", q, k).argmax(-1)[0, 0]        # the permutation crosses key tiles and blocks
            if N >= 64:
                assert bool((pi // 32 != torch.arange(N) // 32).any())
            if N >= 512:
                assert bool((pi // 256 != torch.arange(N) // 256).any())
        if fam == "F3":
            base = make_qkv("F1", B, N, 100 + N)          # the same draws; F3 without dimension 0 is F1 without dimension 0
            for t in (qkv, base):
                t[:, 0:HID:DH] = 0
                t[:, HID:2 * HID:DH] = 0
            assert torch.allclose(ref[:2], ref_full(base)[:2], rtol=0, atol=1e-11)
            qkv = make_qkv(fam, B, N, 100 + N)
        for var in variants:
            for cast in ((lambda t: t), bf16) if var in ("bf16", "mfma") else ((lambda t: t),):
                tol, V = full_tol(cast(qkv), var)
                assert torch.isfinite(tol).all() and bool((tol > 0).all())
                if fam != "F3":
                    cap = CAP_BF16 if var in ("bf16", "mfma") else CAP_F32
                    assert bool((tol <= cap * V).all()), (fam, var, float((tol / V).max()), cap)
        # the loosest tolerance any variant uses at this N: a defect it rejects is rejected by all
        x = bf16(qkv) if {"bf16", "mfma"} & set(variants) else qkv
        ref_x = ref_full(x)
        tol = torch.stack([full_tol(x, var)[0] for var in variants]).amax(0)
        assert not bool(exceeds(ref_x, ref_x, tol).any())
        if fam in ("F1", "F2") and N >= 2:
            for d in caught:
                caught[d] = caught[d] or bool(exceeds(ref_full(x, d), ref_x, tol).any())
        if fam in ("F1", "F2"):
            assert not bool(exceeds(ref_full(x, "partial_max"), ref_x, tol).any())      # (invisible there, as argued above)
        if fam == "F3" and N > 32:
            bad = exceeds(ref_full(x, "partial_max"), ref_x, tol)
            assert bool(bad[2].any()) and not bool(bad[:2].any())
    if N >= 2:
        assert all(caught.values()), caught


@pytest.mark.parametrize("N", LINEAR_N)
def test_linear_families_bounds_and_power(N):
    B = 3
    caught = {d: False for d in ("swap_v", "drop_last")}
    for fam in ("F1", "F2", "F3"):
        qkv = bf16(make_qkv(fam, B, N, 200 + N, linear=True))
        ref = ref_linear(qkv)
        assert torch.isfinite(ref).all()
        for var in ("f32", "bf16"):
            tol, V = linear_tol(qkv, var)
            assert torch.isfinite(tol).all() and bool((tol > 0).all())
            if fam != "F3":
                assert bool((tol <= (CAP_BF16 if var == "bf16" else CAP_F32) * V).all())
            assert bool((ref.reshape(B, HEADS, DH, N).abs() <= SCALE * V / N * (1 + 1e-12)).all())   # the scale of the bound
        if fam == "F2":
            k = heads(qkv.double())[1]
            # (one pixel holds e^12 against ~1.6 N for the rest: peaked over n, if not a pointer at the largest N)
            assert N == 1 or float(k.softmax(-1).amax(-1)[:, :, list(POINTED_COLUMNS)].min()) > 0.25
        tol = linear_tol(qkv, "bf16")[0]
        if fam in ("F1", "F2") and N >= 2:
            for d in caught:
                caught[d] = caught[d] or bool(exceeds(ref_linear(qkv, d), ref, tol).any())
    if N >= 2:
        assert all(caught.values()), caught


def test_f4_references_are_non_finite_where_they_must_be():
    B, N, P = 3, 129, F4_POS
    for linear, ref_fn in ((False, ref_full), (True, ref_linear)):
        ok = ref_fn(make_qkv("F4_nan_v", B, N, 5).nan_to_num(0.0)).reshape(B, HEADS, DH, N)
        r = ref_fn(make_qkv("F4_nan_v", B, N, 5)).reshape(B, HEADS, DH, N)
        want = torch.zeros_like(r, dtype=torch.bool)
        want[B - 1, P["h"], P["e"]] = True
        assert torch.equal(torch.isnan(r), want) and torch.isfinite(ok).all()
        r = ref_fn(make_qkv("F4_nan_k", B, N, 5)).reshape(B, HEADS, DH, N)
        want = torch.zeros_like(want)
        want[B - 1, P["h"]] = True
        assert torch.equal(torch.isnan(r), want)
        r = ref_fn(make_qkv("F4_inf_v", B, N, 5)).reshape(B, HEADS, DH, N)
        want = torch.zeros_like(want)
        want[B - 1, P["h"], P["e"]] = True
        assert torch.equal(torch.isposinf(r), want) and not torch.isnan(r).any()
        # every probability of the soft base stays far above the 2^-25 at which an f16 half is zero
        if not linear:
            q, k, _ = heads(make_qkv("F4_inf_v", B, 1024, 5).double())
            assert float(torch.einsum("bhdi,bhdj->bhij", q * SCALE, k).softmax(-1).min()) > 2.0 ** -20


@pytest.mark.parametrize("dtype,C", [("f32", c) for c in LN_C_F32] + [("bf16", c) for c in LN_C_BF16])
def test_layernorm_bounds_reject_a_one_pass_variance(dtype, C):
    """the cancellation rows (100 + 0.01 N(0,1)): E[x^2] - E[x]^2 in float32 loses all of the variance, and the bound notices"""
    for name, x, g, res in layernorm_inputs(1000, C, dtype):
        ref = ref_layernorm(x, g, res)
        tol = layernorm_tol(x, g, ref, dtype, res)
        fin = torch.isfinite(ref)
        assert torch.isfinite(tol[fin]).all()
        if name == "cancel" and dtype == "f32":
            xf = x.float()
            mean = xf.mean(1, keepdim=True)
            var = ((xf * xf).mean(1, keepdim=True) - mean * mean).clamp(min=0)
            one_pass = ((xf - mean) * (var + 1e-5).rsqrt() * g).double() + (0 if res is None else res.double())
            assert bool(((one_pass - ref).abs() > tol).any())


def layernorm_inputs(M, C, dtype, seed=0):
    """(name, x, g, residual): N(0,1); 100 + 0.01 N(0,1); N(0,1) with a constant row and a row holding one NaN"""
    g = torch.Generator().manual_seed(31 * C + M + seed)
    cast = bf16 if dtype == "bf16" else (lambda t: t)
    gain = 1 + 0.2 * torch.randn(C, generator=g)
    out = []
    for name in ("normal", "cancel", "rows"):
        x = torch.randn((M, C), generator=g)
        if name == "cancel":
            x = 100 + 0.01 * x
        if name == "rows":
            x[M // 2] = 0.7
            x[M // 3, C // 2] = float("nan")
        for res in (None, torch.randn((M, C), generator=g)):
            out.append((name + ("+res" if res is not None else ""), cast(x), gain, None if res is None else cast(res)))
    return out


@pytest.mark.parametrize("C", (64, 128, 256))
def test_block_emulation_stays_under_its_caps(C):
    """a loose emulation would widen the GPU test's bound (3 x its maximum, 2 x its mean): it may not exceed 0.05 / 0.006"""
    for B in (1, 3):
        for N in BLOCK_N_BF16:
            _, x, ref, emax, emean = block_case(C, B, N, "R", "bf16")
            assert emax <= EMU_CAP_MAX and emean <= EMU_CAP_MEAN, (C, B, N, emax, emean)
            assert float((ref - x).abs().max()) < 8.0


@pytest.mark.parametrize("C", (64, 128))
def test_split_emulation_is_at_float32_level(C):
    for N in BLOCK_N_SPLIT:
        _, _, ref, emax, _ = block_case(C, 3, N, "R", "f16x3")
        assert 0 < emax <= 5e-6 * max(1.0, float(ref.abs().max())), (C, N, emax)


@pytest.mark.parametrize("C", (64, 128, 256))
def test_bound_edge_family_reaches_the_static_bound(C):
    W = block_weights(C, 1000 + C, "E")
    bounds = static_bounds(W["w_qkv"], W["norm_g"])
    assert float(bounds.max()) <= STATIC_LIMIT and float(bounds.min()) > 55.0, (float(bounds.min()), float(bounds.max()))
    x = bf16(block_x(W, 3, 100, 7 * C + 139, "E"))
    k = torch.einsum("oc,bcn->bon", bf16(fold_qkv(W["w_qkv"], W["norm_g"])).double(), bf16(_ln64(x.double(), 1)))[:, HID:2 * HID]
    assert float(k.abs().max()) >= 0.9 * 56.0, float(k.abs().max())
    # the realistic family keeps its bound at C = 64 (so its static path runs) and loses it at C = 256 (PRG_E_INVALID, asserted
    # by the GPU test for whichever weights exceed the limit)
    R = static_bounds(*[block_weights(C, 1000 + C)[n] for n in ("w_qkv", "norm_g")])
    if C != 128:
        assert (float(R.max()) <= STATIC_LIMIT) == (C == 64), float(R.max())
