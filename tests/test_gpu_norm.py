"""The GroupNorm passes of blocks.hip, each alone through its test hook against the float64 references of tests/test_norm_refs.py,
whose docstring derives every tolerance used here: launch_gn_stats<float / bf16> slab by slab (prg_debug_gn_stats), gn_coeff_kernel
with every conditioning form and lanes-per-group layout (prg_debug_gn_coeff), cond_fold_kernel with its accumulator-clearing loop,
gn_coeff_acc_kernel and affine_silu_fold_kernel (prg_debug_gn_fold), and affine_silu_kernel<float / bf16> (prg_debug_affine_silu).
Every case prints its largest error / tolerance and asserts it <= 1.

The slab-cap case (HW = 8200 at psub = 1) asks for 1025 slabs of 8 pixels, is cut to 1024, and so takes slabs of 9 pixels, of which
912 cover the image: nsplit = 912 is what launch_gn_stats' formula gives and what the test asserts.  The 16x16, C = 64 fold pass,
proposed as one block per image, has 2048 vectors per image: two 1024-vector blocks; HW = 128 is added for the one-block launch.

Observed on an MI355X, largest error / tolerance per kernel and family (all 54 cases pass; the module takes 7.5 s as a process of
its own, 4.3 - 4.9 s of it the 4096-vector fold pass with its references over 16.8 M elements, every other case under 0.3 s):
  gn_stats     bf16 (float32 accumulation) sums 0 .. 0.015, squares 0.001 .. 0.11: the bound is the worst case of a chain of `depth`
               additions; float (float64 accumulation, one rounding per slab) sums 0.42 .. 0.999, squares 0.075 .. 0.996: the bound
               is that one rounding.  nsplit as the formula says in all 14 cases (1, 3, 5, 9, 10, 912).  Beside a +Inf: 0.98 (float),
               0.054 (bf16), and non-finite entries in exactly the slab and group of the +Inf.
  gn_coeff     16 layouts x 5 conditioning forms 0.32 .. 0.99 (largest at C = 1024); the constant image (clamp) 0.68 .. 0.78, with
               A = float((1e-5)^-1/2) gamma bit for bit; |mean| / std = 2^8 0.52 .. 0.63.
  gn_coeff_acc 0.43 .. 0.91, NaN in exactly the poisoned group's channels of its image, P, Q shared and per image.
  cond_fold    P, Q 0.90 .. 0.997 at every zero_words (0, 500, 2304, 3304); every float of pq between the entries untouched; exactly
               zero_words words cleared and the 64 behind them unchanged in all 16 launches; the tables made from the folded P, Q
               through the per-image stride 0.45 .. 0.99.
  affine_silu_fold  0.999 .. 1.000 in all five launch shapes, with and without residual (half a bf16 ulp is the dominant term and
               some element of every tensor comes close to it), the float32 reference on both images of the large case 0.999 .. 1.000;
               in place bit-identical to out of place everywhere.
  affine_silu  float 0.65 .. 0.96, bf16 0.999 .. 1.000; in place bit-identical; -Inf gives NaN in both forms, nothing else changes;
               16 778 240 vectors in one launch (the grid-stride loop's second iteration) bit-identical to the two single-image
               launches, float and bf16.
No case failed at any point: these tests found no defect in the kernels.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from pointreggpt_amd import _lib
from test_conv_fused_refs import POISON, fold_inputs
from test_norm_refs import (COEFF_FORMS, COEFF_LAYOUT, PATTERN, STATS_CASES, apply_input, apply_reference, coeff_input, coeff_reference,
                            cond_fold_input, cond_fold_reference, fold_tables, gen, ratio, stats_input, stats_reference, stats_split, VEC,
                            zero_expected)

pytestmark = pytest.mark.gpu

GUARD = 1024
DT = {"f32": _lib.PRG_F32, "bf16": _lib.PRG_BF16}


def dev(t, dtype=torch.float32):
    return t.to(dtype).contiguous().cuda()


def guarded(n, fill=-7.0):
    """a device buffer of n floats with GUARD floats either side: (whole tensor, pointer to the payload)"""
    big = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device="cuda")
    return big, big.data_ptr() + 4 * GUARD


def payload(big, n, fill=-7.0):
    big = big.cpu()
    assert bool((big[:GUARD] == fill).all()) and bool((big[GUARD + n:] == fill).all()), "guard floats were written"
    return big[GUARD:GUARD + n]


def report(label, **q):
    print(f"{label}: largest error / tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, (label, q)


# ------------------------------------------------------------------------------------------------------------------------------
# gn_stats
# ------------------------------------------------------------------------------------------------------------------------------
def run_stats(x, G, dtype):
    lib = _lib.load()
    B, Cc, HW = x.shape
    dx = dev(x)
    cap = B * 1024 * G * 2
    big, p = guarded(cap)
    ns = C.c_int(-1)
    _lib.check(lib.prg_debug_gn_stats(_lib.ptr(dx), p, C.byref(ns), B, Cc, HW, G, DT[dtype], _lib.stream_ptr()), "prg_debug_gn_stats")
    out = payload(big, cap)
    n = B * ns.value * G * 2
    assert bool((out[n:] == -7.0).all()), "floats behind the slabs were written"
    return ns.value, out[:n].reshape(B, ns.value, G, 2).double()


@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: f"{c[0]} {c[1]} C={c[3]} HW={c[4]} G={c[5]}")
def test_gn_stats_slab_by_slab(case):
    name, dtype, B, Cc, HW, G = case
    x = stats_input(STATS_CASES.index(case), B, Cc, HW, dtype)
    want_ns, ref, tol = stats_reference(x, G, dtype)
    assert want_ns == stats_split(HW, Cc, VEC[dtype])[0]
    slab, psub = stats_split(HW, Cc, VEC[dtype])[1:]
    if "cap" in name:                                 # 1025 slabs of 8 pixels asked for, 1024 allowed: slabs of 9, and 912 of those
        assert psub == 1 and -(-HW // 8) > 1024 and slab == 9 and want_ns == -(-HW // 9)
    if "one slab" in name:
        assert want_ns == 1
    if "short last slab" in name:
        assert want_ns > 1 and want_ns * slab > HW
    if "HW < psub" in name:
        assert HW < psub
    ns, got = run_stats(x, G, dtype)
    assert ns == want_ns, (ns, want_ns)
    report(f"gn_stats {dtype} {name} (B, C, HW, G) = {(B, Cc, HW, G)} nsplit {ns}", sums=ratio(got[..., 0], ref[..., 0], tol[..., 0]),
           squares=ratio(got[..., 1], ref[..., 1], tol[..., 1]))


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_gn_stats_an_infinity_stays_in_its_slab(dtype):
    B, Cc, HW, G = 3, 64, 1093, 8
    x = stats_input(50, B, Cc, HW, dtype)
    ns, slab, _ = stats_split(HW, Cc, VEC[dtype])
    pix, ch = 2 * slab + 1, 19
    x[1, ch, pix] = float("inf")
    got_ns, got = run_stats(x, G, dtype)
    assert got_ns == ns
    bad = ~torch.isfinite(got)
    want = torch.zeros_like(bad)
    want[1, pix // slab, ch // (Cc // G)] = True
    assert bool((bad == want).all()), "non-finite entries exactly in the slab and group of the +Inf"
    x[1, ch, pix] = 0.0
    _, ref, tol = stats_reference(x, G, dtype)
    keep = ~want
    report(f"gn_stats {dtype} +Inf in image 1: every other entry", sums=ratio(got[keep], ref[keep], tol[keep]))


# ------------------------------------------------------------------------------------------------------------------------------
# gn_coeff
# ------------------------------------------------------------------------------------------------------------------------------
def run_coeff(d):
    lib = _lib.load()
    B, Cc = d["B"], d["C"]
    keep = [dev(d["slabs"]), dev(d["gamma"]), dev(d["beta"])]
    pa = pb = None
    na = nb = 0
    if d["ss_a"] is not None:
        a = dev(d["ss_a"].reshape(-1))
        keep.append(a)
        pa, na = a.data_ptr() + 4 * d["ss_off"], a.numel() - d["ss_off"]
    if d["ss_b"] is not None:
        b = dev(d["ss_b"].reshape(-1))
        keep.append(b)
        pb, nb = b.data_ptr() + 4 * d["ss_off"], b.numel() - d["ss_off"]
    row = C.c_int(d["row"]) if d["row"] is not None else None
    out = torch.full((2, B + 2, Cc), -7.0, dtype=torch.float32, device="cuda")             # a guard row either side of A and of Bc
    rc = lib.prg_debug_gn_coeff(_lib.ptr(keep[0]), d["ns"], _lib.ptr(keep[1]), _lib.ptr(keep[2]), pa, d["ss_a_stride"], na, pb, d["ss_b_stride"], nb,
                                C.byref(row) if row is not None else None, d["row_stride"], out[0, 1].data_ptr(), out[1, 1].data_ptr(), B, d["HW"],
                                Cc, d["G"], _lib.stream_ptr())
    _lib.check(rc, "prg_debug_gn_coeff")
    out = out.cpu()
    assert bool((out[:, 0] == -7.0).all()) and bool((out[:, -1] == -7.0).all()), "guard rows were written"
    return out[0, 1:-1].double(), out[1, 1:-1].double()


def check_coeff(label, d):
    a, b, ta, tb = coeff_reference(d)
    ga, gb = run_coeff(d)
    return ratio(ga, a, ta), ratio(gb, b, tb)


@pytest.mark.parametrize("layout", COEFF_LAYOUT, ids=lambda l: f"B{l[0]} C{l[1]} G{l[2]} nsplit{l[3]}")
def test_gn_coeff_layouts_and_conditioning(layout):
    B, Cc, G, ns = layout
    worst = {}
    for form in COEFF_FORMS:
        d = coeff_input(COEFF_LAYOUT.index(layout), B, Cc, G, 64, ns, form)
        qa, qb = check_coeff(form, d)
        worst[form.replace(" ", "_")] = max(qa, qb)
    report(f"gn_coeff (B, C, G, nsplit) = {layout}", **worst)


@pytest.mark.parametrize("edge", ("constant", "large_mean"))
def test_gn_coeff_edges(edge):
    worst = {}
    for G, ns in ((1, 65), (8, 16), (64, 33)):
        d = coeff_input(7, 2, 64, G, 64, ns, "a_img", edge=edge)
        qa, qb = check_coeff(edge, d)
        worst[f"G{G}"] = max(qa, qb)
        if edge == "constant":                      # the clamp: rstd = (1e-5)^-1/2 rounded once, so A is that times gamma to one rounding
            rstd = torch.tensor(1e-5, dtype=torch.float64) ** -0.5
            plain = run_coeff(dict(d, ss_a=None))[0]
            assert torch.equal(plain.float(), (rstd.float() * d["gamma"])[None].expand(2, -1))
    report(f"gn_coeff {edge}", **worst)


# ------------------------------------------------------------------------------------------------------------------------------
# gn_fold
# ------------------------------------------------------------------------------------------------------------------------------
def run_fold(B, Cc=0, HW=0, G=0, acc=None, P=None, Q=None, cond=None, zero_words=0, use_entry=0, output=_lib.GF_TABLES, x=None, residual=None,
             in_place=0):
    lib = _lib.load()
    keep = []

    def d_(t, dtype=torch.float32):
        t = dev(t, dtype)
        keep.append(t)
        return t.data_ptr()

    a = _lib.GnFoldC(B=B, C=Cc, HW=HW, groups=G, output=output, in_place=in_place, use_entry=use_entry)
    got = {}
    if acc is not None:
        a.acc = d_(acc, torch.int64)
    if cond is None:
        a.p, a.q, a.pq_per_image = d_(P), d_(Q), int(P.dim() == 2)
    else:
        ent = np.array(cond["entries"], dtype=np.int64)
        keep.append(ent)
        a.entries, a.n_entries, a.ss_total = ent.ctypes.data, len(ent), cond["ss_total"]
        a.flat, a.flat_floats = d_(cond["flat"]), cond["flat"].numel()
        a.ss_a, a.ss_a_stride, a.ss_a_floats = d_(cond["ss_a"]), cond["ss_a_stride"], cond["ss_a"].numel()
        if cond["ss_b"] is not None:
            a.ss_b, a.ss_b_stride, a.ss_b_floats = d_(cond["ss_b"]), cond["ss_b_stride"], cond["ss_b"].numel()
        if cond["row"] is not None:
            row = np.array([cond["row"]], dtype=np.int32)
            keep.append(row)
            a.row, a.row_stride = row.ctypes.data, cond["row_stride"]
        pq = dev(cond["pq"])
        zero = torch.full((zero_words + 64,), 3, dtype=torch.int64, device="cuda")
        a.pq, a.zero_out, a.zero_words = pq.data_ptr(), zero.data_ptr(), zero_words
    if output == _lib.GF_TABLES:
        coef = torch.full((2, B + 2, Cc), -7.0, dtype=torch.float32, device="cuda")
        a.coef_a, a.coef_b = coef[0, 1].data_ptr(), coef[1, 1].data_ptr()
    if output == _lib.GF_APPLY:
        n = B * Cc * HW
        a.x = d_(x)
        if residual is not None:
            a.residual = d_(residual)
        big, a.out = guarded(n)
    _lib.check(lib.prg_debug_gn_fold(C.byref(a), _lib.stream_ptr()), "prg_debug_gn_fold")
    if cond is not None:
        got.update(pq=pq.cpu().double(), zero=zero.cpu().numpy())
    if output == _lib.GF_TABLES:
        coef = coef.cpu()
        assert bool((coef[:, 0] == -7.0).all()) and bool((coef[:, -1] == -7.0).all()), "guard rows were written"
        got.update(A=coef[0, 1:-1].double(), Bc=coef[1, 1:-1].double())
    if output == _lib.GF_APPLY:
        got["out"] = payload(big, n).reshape(B, Cc, HW).double()
    return got


@pytest.mark.parametrize("per_image", (0, 1), ids=("pq_stride=0", "pq_stride=2C"))
@pytest.mark.parametrize("Cc", (64, 1024))
def test_fold_tables_from_accumulators(Cc, per_image):
    B, G, HW = 3, 8, 144
    f = fold_inputs(gen(60 + per_image), B, G, Cc, HW, poison=(1, 3))
    if per_image:
        s = torch.tensor([[1.0], [-0.5], [1.75]])
        f = dict(acc=f["acc"], P=(f["P"][None] * s).contiguous(), Q=(f["Q"][None] + s).contiguous())
    A, Bc, dA, dB = fold_tables(f, G, Cc, HW)
    got = run_fold(B, Cc, HW, G, acc=f["acc"], P=f["P"], Q=f["Q"])
    cpg = Cc // G
    want_nan = torch.zeros(B, Cc, dtype=torch.bool)
    want_nan[1, 3 * cpg:4 * cpg] = True
    assert int(f["acc"][1, 3, 1]) < 0 and int(f["acc"][1, 3, 1]) & ~POISON > 0
    assert bool((torch.isnan(got["A"]) == want_nan).all()) and bool((torch.isnan(got["Bc"]) == want_nan).all()), "NaN exactly in the poisoned group"
    report(f"gn_coeff_acc C {Cc} per-image P, Q {per_image}", A=ratio(got["A"], A, dA), Bc=ratio(got["Bc"], Bc, dB))


@pytest.mark.parametrize("with_b,with_row", ((False, False), (True, False), (True, True), (False, True)))
def test_cond_fold_and_its_zero_loop(with_b, with_row):
    B = 3
    d = cond_fold_input(70, B, with_b, with_row)
    ref, tol = cond_fold_reference(d)
    n = len(d["entries"])
    worst = {}
    for zw in (500, n * B * 256, n * B * 256 + 1000, 0):
        got = run_fold(B, cond=d, zero_words=zw, output=_lib.GF_NONE)
        worst[f"zero_words_{zw}"] = ratio(got["pq"], ref, tol)                    # (tolerance 0 between the entries: bit for bit)
        want = zero_expected(zw)
        wrong = int((got["zero"] != want).sum())
        assert wrong == 0, f"zero_words {zw}: {wrong} words differ: exactly zero_words words are cleared and the 64 behind keep {PATTERN:#x}"
    report(f"cond_fold ss_b {with_b} row {with_row}: P, Q", **worst)
    # the tables of entry 2 (C = 512) through the folded P, Q: gn_coeff_acc on a per-image stride of ss_total
    off, Cc, _, _ = d["entries"][2]
    G, HW = 8, 64
    f = fold_inputs(gen(71), B, G, Cc, HW)
    got = run_fold(B, Cc, HW, G, acc=f["acc"], cond=d, zero_words=64, use_entry=2)
    per = dict(acc=f["acc"], P=ref[:, off:off + Cc], Q=ref[:, off + Cc:off + 2 * Cc])
    A, Bc, dA, dB = fold_tables(per, G, Cc, HW)
    rstd, mr, _, _ = fold_tables(dict(acc=f["acc"], P=torch.ones(Cc), Q=torch.zeros(Cc)), G, Cc, HW)     # (rstd, -mean rstd)
    dP, dQ = tol[:, off:off + Cc], tol[:, off + Cc:off + 2 * Cc]
    report(f"cond_fold ss_b {with_b} row {with_row}: tables of entry 2", A=ratio(got["A"], A, dA + rstd.abs() * dP),
           Bc=ratio(got["Bc"], Bc, dB + dQ + mr.abs() * dP))


# (B, C, HW, G, what)
FOLD_PASS = [(2, 64, 256, 8, "1024-vector blocks, two per image"), (2, 64, 128, 8, "1024-vector blocks, one per image"),
             (2, 64, 1092, 8, "nine blocks per image, ragged last"), (2, 512, 16384, 8, "4096-vector blocks, four iterations"),
             (17000, 8, 4, 1, "the 16384 / B cap")]


@pytest.mark.parametrize("case", FOLD_PASS, ids=lambda c: c[4])
def test_fold_pass(case):
    B, Cc, HW, G, what = case
    per_img = HW * Cc // 8
    small = per_img * B < 2 << 20
    assert small == ("4096" not in what)
    f = fold_inputs(gen(80), B, G, Cc, HW)
    x, _, _, r = apply_input(81, B, Cc, HW, "bf16", True)
    big = B * Cc * HW > 1 << 22
    worst = {}
    for res in (None, r):
        got = run_fold(B, Cc, HW, G, acc=f["acc"], P=f["P"], Q=f["Q"], output=_lib.GF_APPLY, x=x, residual=res)
        inp = run_fold(B, Cc, HW, G, acc=f["acc"], P=f["P"], Q=f["Q"], output=_lib.GF_APPLY, x=x, residual=res, in_place=1)
        assert torch.equal(got["out"], inp["out"]), "the in-place launch differs from the out-of-place one"
        tag = "residual" if res is not None else "plain"
        imgs = [0] if big else list(range(B))
        A, Bc, dA, dB = fold_tables(f, G, Cc, HW, imgs)
        ref, tol = apply_reference(x[imgs], A, Bc, dA, dB, None if res is None else res[imgs], "bf16")
        worst[tag] = ratio(got["out"][imgs], ref, tol)
        if big:                                   # float32 on every image, the tolerance's float32 part doubled
            A, Bc, dA, dB = fold_tables(f, G, Cc, HW)
            ref, tol = apply_reference(x.float(), A.float(), Bc.float(), dA, dB, None if res is None else res.float(), "bf16", scale=2.0)
            worst[tag + "_f32"] = ratio(got["out"], ref, tol)
    report(f"affine_silu_fold {what} (B, C, HW) = {(B, Cc, HW)}, in place bit-identical", **worst)


# ------------------------------------------------------------------------------------------------------------------------------
# affine_silu
# ------------------------------------------------------------------------------------------------------------------------------
def run_affine(x, A, Bc, residual, dtype, in_place=0):
    """x, residual (B, C, HW), A, Bc (B, C): CPU tensors, or device float32 tensors (the result then stays on the device)"""
    lib = _lib.load()
    B, Cc, HW = x.shape
    on_dev = x.is_cuda
    dx, dA, dB = (t if on_dev else dev(t) for t in (x, A, Bc))
    dr = None if residual is None else residual if on_dev else dev(residual)
    n = B * Cc * HW
    big, p = guarded(n)
    _lib.check(lib.prg_debug_affine_silu(_lib.ptr(dx), _lib.ptr(dA), _lib.ptr(dB), _lib.ptr(dr), p, B, Cc, HW, DT[dtype], in_place, _lib.stream_ptr()),
               "prg_debug_affine_silu")
    if on_dev:
        assert bool((big[:GUARD] == -7.0).all()) and bool((big[GUARD + n:] == -7.0).all()), "guard floats were written"
        return big[GUARD:GUARD + n].reshape(B, Cc, HW)
    return payload(big, n).reshape(B, Cc, HW).double()


# (B, C, HW): below one block of 1024 vectors; no multiple of 1024 vectors; one vector per pixel; three vectors per pixel
AFFINE = {"bf16": [(2, 64, 50), (3, 64, 300), (2, 8, 1500), (3, 24, 1001)], "f32": [(2, 64, 25), (3, 64, 150), (2, 4, 1500), (3, 12, 1001)]}


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_affine_silu(dtype):
    worst = {}
    for B, Cc, HW in AFFINE[dtype]:
        x, A, Bc, r = apply_input(90, B, Cc, HW, dtype, True)
        z = torch.zeros(B, Cc, dtype=torch.float64)
        for res in (None, r):
            got = run_affine(x, A, Bc, res, dtype)
            assert torch.equal(got, run_affine(x, A, Bc, res, dtype, in_place=1)), "the in-place launch differs from the out-of-place one"
            ref, tol = apply_reference(x, A.double(), Bc.double(), z, z, res, dtype)
            worst[f"C{Cc}_HW{HW}_{'residual' if res is not None else 'plain'}"] = ratio(got, ref, tol)
    report(f"affine_silu {dtype}, in place bit-identical", **worst)


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_affine_silu_minus_infinity_gives_nan(dtype):
    # u = -Inf: the float form is -Inf / (1 + expf(Inf)) = -Inf / Inf, the bf16 form -Inf * rcp(1 + exp2(Inf)) = -Inf * 0: NaN both,
    # as the float64 formula u * sigmoid(u) = -Inf * 0 gives (not -0)
    B, Cc, HW = 2, 24, 40
    x, A, Bc, _ = apply_input(91, B, Cc, HW, dtype, False)
    x[1, 5, 7] = float("-inf")
    A[1, 5] = 1.25
    z = torch.zeros(B, Cc, dtype=torch.float64)
    ref, tol = apply_reference(x, A.double(), Bc.double(), z, z, None, dtype)
    assert bool(torch.isnan(ref[1, 5, 7])) and int(torch.isnan(ref).sum()) == 1
    got = run_affine(x, A, Bc, None, dtype)
    assert bool(torch.isnan(got[1, 5, 7])) and int(torch.isnan(got).sum()) == 1
    report(f"affine_silu {dtype} with one -Inf: NaN there, everything else", out=ratio(got, ref, tol))


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_affine_silu_grid_stride_loop(dtype):
    # more than 16384 x 1024 vectors in one launch: the grid is capped and the four-deep loop runs twice for the first threads.  Each
    # image alone is half of that: one iteration, the regime test_affine_silu validates.  Same data, so bit for bit.
    B, Cc = 2, 64
    HW = (16384 * 1024 // 2 + 512) // (Cc // VEC[dtype])
    assert B * HW * (Cc // VEC[dtype]) > 16384 * 1024 >= HW * (Cc // VEC[dtype])
    g = torch.Generator(device="cuda").manual_seed(92)
    x = torch.randn(B, Cc, HW, generator=g, device="cuda")
    r = torch.randn(B, Cc, HW, generator=g, device="cuda")
    A = 1.0 + 0.3 * torch.randn(B, Cc, generator=g, device="cuda")
    Bc = 0.5 * torch.randn(B, Cc, generator=g, device="cuda")
    both = run_affine(x, A, Bc, r, dtype)
    for b in range(B):
        one = run_affine(x[b:b + 1].contiguous(), A[b:b + 1].contiguous(), Bc[b:b + 1].contiguous(), r[b:b + 1].contiguous(), dtype)
        assert torch.equal(both[b:b + 1], one), f"image {b} of the two-image launch differs from its own launch"
        del one
    assert bool(torch.isfinite(both).all()) and float(both.abs().max()) > 1.0
    print(f"affine_silu {dtype} {B * HW * (Cc // VEC[dtype])} vectors in one launch: bit-identical to the two single-image launches")
