"""One float32-storage convolution (f16x3: the split-f16 kernels of conv_split.hip / conv_split512.hip; fp32: conv.hip with T = float)
through launch_conv with the fused options the forward pass sets on it (prg_debug_conv_fused, storage 1 / 2) against the float64
references of tests/test_conv_fused_f32_refs.py, whose docstring derives every tolerance used here: two sources, statistics of the
output as slabs (and the separate pass when nothing fuses), the table prologue, and the 1x1 epilogues (plain and table residual, in
place or not).  The hook, the guard floats, Refs and the single-source helper are tests/test_gpu_conv_fused.py's.

Every case names the kernel and tile the dispatch (conv_choose.cpp) is expected to choose, asserts the family and tile the hook
reports and (nsplit, stats_pass) from that family's slab formula, and prints its largest error / tolerance.  Where statistics are
fused, every slab is compared with the reference's sums over that slab's pixels, not only the slabs' sum.

Shapes: the smallest that select each kernel by default.  (2, 64, 64, 128, 16, 16) with groups = 1 runs conv3x3_split_ws_kernel
without statistics, but with them both slab rules decline (a group of 128 channels spans two waves and two 64-channel tiles), so it
runs the 8x16 split halo tile and the separate pass; (2, 64, 0, 64, 16, 32) with groups = 1 is the whole-tile group tile_fuse still
takes.  The prologue on the 4x32 split halo tile runs at (2, 64, 0, 128, 12, 32), not at the proposed (2, 64, 0, 64, 12, 32):
conv_supports_prologue<float> (what resblock() asks, and the hook) answers for the fp32 halo tiles, which take H % 8 != 0 only with
Cout % 128 == 0; with H = 12 the split dispatch then still declines the 16- and 8-row kernels and runs the 4x32 tile with two
channel tiles.  In fp32, (2, 64, 64, 64, 12, 32) has no halo tile (H % 8 != 0) and runs the gather kernel with three slabs per image.
Groups of 24 or 48 channels (Cout = 192 / 384 with 8 groups) divide neither a 64- nor a 128-channel tile: the tile reductions give a tile
bn / cpg whole groups from its first channel, so tile_fuse has to decline them.  It did not before this module existed: the fused
slabs held other channels' sums and left two groups unwritten (sums 2e4 tolerances off, on the fp32 and the split halo kernel
alike, and on the bf16 halo kernel by the same code).  conv_choose.cpp now asks bn % cpg == 0.  launch_gn_stats has no kernel for such
widths either (C / vec a power of two), so a launch that asks for their statistics now fails with that error instead of returning
wrong sums: test_groups_that_straddle_a_channel_tile_are_never_fused pins it, in the three storage modes.
Large batches (w512: one tile per CU; p64: 256 tiles): four distinct images, image b a copy of image b % 4; the float64 reference
runs on the four, every copy's output, slabs, sums and coefficients must equal its original's bit for bit (B - 4 copies per case
are not compared against float64: 252 on a 256-CU part for w512, 60 for p64).  No kernel's arithmetic depends on the tile's place.
Zero sources: fp32 on the halo tile and the 1x1 is bit-identical to the single-source call (a zero source's 32-term partials are
exact zeros in the float64 sum); the fp32 gather kernel at 72 + 48 channels regroups its 16-term partials, and every f16x3 kernel
scales a channel's weights by the power of two of max |w| over BOTH sources' columns (weights_host.cpp:209-224), which moves the
subnormal floor of the lo halves when the larger weights belong to the zero source: those agree within 2 tolerances.

Observed on an MI355X (256 CUs), largest error / tolerance per family (all 98 cases pass, the module takes 6 - 7 s):
  output      f16x3 3x3: split halo 0.0030 .. 0.0053, split ws 0.0022 .. 0.0032, w512 0.0034, p64 0.0038, gather 0.0037 .. 0.0042; with the
              prologue (tables, border) split halo 0.0022 .. 0.0062, ws 0.0016 .. 0.0041, w512 0.0016 .. 0.0046, p64 0.0024 .. 0.0081;
              forced p64 0.0033 .. 0.0063, forced w512 0.0034 .. 0.0043; 1x1 0.0039 .. 0.010 whatever the epilogue; amplitudes 0.0087 ..
              0.014; rms 2^-16 0.060 .. 0.10 (the 2^-25 floor of the subnormal halves is the bound's leading term there, and the
              kernels use a sixth to a tenth of it); zero sources 0.0033 .. 0.0094.  The bound's leading term is the worst case of
              291 .. 295 float32 roundings; the matrix pipe delivers a few hundredths of it, which is why the planted fault
              "lo half dropped" (tests/test_conv_fused_f32_refs.py) lands at 2.5 .. 3.0 and not far above.
              fp32 3x3: halo 0.012 .. 0.021, gather 0.011 .. 0.013, with the prologue 0.0087 .. 0.019; 1x1 0.011 .. 0.046;
              amplitudes 0.019 .. 0.024, rms 2^-16 0.028 .. 0.029, zero sources 0.013 .. 0.051: the float32 store's half ulp
              against 34 e P.
  slabs       f16x3 fused 8e-5 .. 6.5e-4 (rms 2^-16: 3.6e-3), fp32 fused 4.9e-4 .. 2.9e-3 (1.2e-2).  Two swapped wave rows land at 336
              or more, one slab left out at 1.7e3 (tests/test_conv_fused_f32_refs.py).
  sums        fused 5.5e-5 .. 1.2e-3 (f16x3), 2.8e-4 .. 1.1e-2 (fp32); the separate statistics pass 0.12 .. 0.27 (its reference is the
              returned output, t = 0: it sits at the float32 rounding of the slab).
  coefficients  fused 1.5e-4 .. 1.1e-2 (f16x3), 1.1e-3 .. 5.0e-2 (fp32); statistics pass 0.27 .. 0.65.
  Every copy of the large batches (252 for w512, 60 for p64 per launch) was bit-identical to its original in output, slabs, sums and
  coefficients.  Zero sources: every f16x3 call on a halo tile, ws and the 1x1 came out bit-identical to the single-source call
  (no channel's scale moved with these weights); the gather kernels at 72 + 48 channels differed by at most 0.0028 (f16x3) and 0.010
  (fp32) of two tolerances, as expected of another grouping.
No case failed at any point: these tests found no defect in the float kernels or their dispatch.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from pointreggpt_amd import _lib
from test_conv_fused_f32_refs import conv_reference32, expand, make_case32, ratios32, reference32, storage_of
from test_gpu_conv_fused import OFF, SLABS, Refs, cus, run, single_source  # noqa: F401 (cus: fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------------
# what the dispatch is expected to do
# ------------------------------------------------------------------------------------------------------------------------------
def expected(kernel, tile, shape, groups, stats):
    """((family, th, tw, bm, bn), (nsplit, acc_done, stats_pass)) of `kernel` with tile (th, tw, bn), or (bm, bn) for a gather kernel"""
    B, C0, C1, Cout, H, W = shape
    gather = "igemm" in kernel
    choice = (kernel, 0, 0, tile[0], tile[1]) if gather else (kernel, tile[0], tile[1], 0, tile[2])
    if stats == OFF:
        return choice, (0, 0, 0)
    cpg = Cout // groups
    if gather:                                                    # igemm_tiles: HW / BM slabs when a tile lies inside one image
        fuse, ns = (H * W) % tile[0] == 0 and tile[1] % cpg == 0, (H * W) // tile[0]
    elif kernel in ("split_halo", "halo"):                        # tile_fuse: one slab per tile, whole groups per channel tile
        fuse, ns = tile[2] % cpg == 0, (H // tile[0]) * (W // tile[1])
    else:                                                         # wave_rows_fuse: ws two pixel halves per 8x16 tile; p64 and w512 four
        fuse = cpg <= 64 and cpg & (cpg - 1) == 0                 # wave rows per 16x16 tile
        ns = (H // 8) * (W // 16) * 2 if kernel == "split_ws" else (H // 16) * (W // 16) * 4
    return choice, ((ns, 0, 0) if fuse else (0, 0, 1))


def refs32(d, kernel, skip=()):
    return Refs(d, skip, conv_ref=lambda d_, im, dt: conv_reference32(d_, kernel, im), chunks_of=lambda B: [(torch.float64, list(range(B)))])


def tname(kernel, tile):
    return f"{kernel} {'x'.join(map(str, tile))}"


def check_one(label, d, got, kernel, tile, stats, refs):
    """expectation of the dispatch, every tolerance, and the copies of a large batch"""
    n, B = d["shape"][0], d["launch_B"]
    choice, flags = expected(kernel, tile, (B,) + tuple(d["shape"][1:]), d["groups"], stats)
    label = f"{label} [{tname(kernel, tile)}] stats={stats} expect (nsplit, acc_done, stats_pass) = {flags}"
    assert got["choice"] == choice, (label, got["choice"])
    assert got["flags"] == flags, (label, got["flags"])
    how = None if stats == OFF else ("pass" if flags[2] else "fused")
    if how == "fused":
        assert got["slabs"].shape[1] == flags[0], (label, got["slabs"].shape)
    full = lambda core, g: reference32(d, kernel, tile, stats=how, core=core, from_output=g["out"][core["images"]] if how == "pass" else None)
    worst = refs.check(label, got, full_ref=full, ratio_fn=ratios32)
    if B > n:
        orig = torch.arange(n, B) % n
        for k in ("out", "slabs", "sums", "coef_a", "coef_b"):
            if k in got:
                assert torch.equal(got[k][n:], got[k][orig]), f"{label}: {k} of a copy differs from its original's"
        print(f"{label}: {B - n} copies bit-identical to their originals (not compared against float64)")
    return worst


def check_variants(name, d, kernel, tile, modes=(OFF, SLABS), skip=()):
    """the same conv with statistics off and as slabs: one output, bit for bit"""
    launch = expand(d) if d["launch_B"] != d["shape"][0] else d
    refs = refs32(d, kernel, skip)
    outs = []
    for stats in modes:
        got = run(launch, stats=stats, storage=storage_of(kernel), want_slabs=True)
        check_one(name, d, got, kernel, tile, stats, refs)
        outs.append(got["out"])
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), name + ": the statistics mode changed the output"
    return refs


# ------------------------------------------------------------------------------------------------------------------------------
# 3x3
# ------------------------------------------------------------------------------------------------------------------------------
def cases3(cus):       # name -> (shape, groups, kernel, tile, distinct images, modes)
    both = (OFF, SLABS)
    return {
        # f16x3
        "split halo 8x16x64": ((2, 64, 0, 64, 16, 32), 8, "split_halo", (8, 16, 64), None, both),
        "split halo 8x16x64 groups=1": ((2, 64, 0, 64, 16, 32), 1, "split_halo", (8, 16, 64), None, both),
        "split halo 4x32x64 two-source": ((2, 64, 64, 64, 12, 32), 8, "split_halo", (4, 32, 64), None, both),
        "split ws 8x16x128 two-source": ((2, 64, 64, 128, 16, 16), 8, "split_ws", (8, 16, 128), None, both),
        "split ws groups=1 no statistics": ((2, 64, 64, 128, 16, 16), 1, "split_ws", (8, 16, 128), None, (OFF,)),
        "split ws groups=1 declines": ((2, 64, 64, 128, 16, 16), 1, "split_halo", (8, 16, 64), None, (SLABS,)),
        "split ws two channel tiles": ((1, 128, 64, 256, 8, 32), 8, "split_ws", (8, 16, 128), None, both),
        "w512": ((cus, 64, 64, 128, 16, 16), 8, "split_w512", (16, 16, 128), 4, both),
        "p64": ((64, 64, 64, 64, 32, 32), 8, "split_p64", (16, 16, 64), 4, both),
        "split gather fused": ((3, 72, 48, 64, 16, 8), 8, "split_igemm", (128, 64), None, both),
        "split gather separate pass": ((3, 72, 48, 64, 12, 12), 8, "split_igemm", (128, 64), None, both),
        # fp32
        "halo 8x32x64": ((2, 64, 0, 64, 16, 32), 8, "halo", (8, 32, 64), None, both),
        "halo 8x32x64 two-source": ((2, 64, 64, 64, 16, 32), 8, "halo", (8, 32, 64), None, both),
        "halo 8x16x64 two-source": ((2, 64, 64, 64, 16, 16), 8, "halo", (8, 16, 64), None, both),
        "halo 4x32x128 two-source": ((1, 128, 64, 128, 8, 32), 8, "halo", (4, 32, 128), None, both),
        "halo 8x16x128 two-source": ((2, 64, 64, 128, 16, 16), 8, "halo", (8, 16, 128), None, both),
        "halo 8x16x128 groups=1": ((2, 64, 64, 128, 16, 16), 1, "halo", (8, 16, 128), None, both),
        "gather fused": ((3, 72, 48, 64, 16, 8), 8, "igemm", (128, 64), None, both),
        "gather three slabs": ((2, 64, 64, 64, 12, 32), 8, "igemm", (128, 64), None, both),
        "gather separate pass": ((3, 72, 48, 64, 12, 12), 8, "igemm", (128, 64), None, both),
    }


CASES3 = ["split halo 8x16x64", "split halo 8x16x64 groups=1", "split halo 4x32x64 two-source", "split ws 8x16x128 two-source",
          "split ws groups=1 no statistics", "split ws groups=1 declines", "split ws two channel tiles", "w512", "p64", "split gather fused",
          "split gather separate pass", "halo 8x32x64", "halo 8x32x64 two-source", "halo 8x16x64 two-source", "halo 4x32x128 two-source",
          "halo 8x16x128 two-source", "halo 8x16x128 groups=1", "gather fused", "gather three slabs", "gather separate pass"]


def case3(name, cus, family="normal", seed=0, batch=None):
    shape, groups, kernel, tile, distinct, modes = cases3(cus)[name]
    if batch:
        shape = (batch,) + shape[1:]
    return make_case32(shape, groups=groups, family=family, seed=seed, distinct=distinct), kernel, tile, modes


@pytest.mark.parametrize("name", CASES3)
def test_conv3x3_sources_and_statistics(name, cus):
    d, kernel, tile, modes = case3(name, cus, seed=100 + CASES3.index(name))
    check_variants(name, d, kernel, tile, modes)


def cases_pro(cus):    # single-source shapes with the table prologue: (shape, kernel, tile, distinct images)
    return {
        "split halo 8x16x64": ((2, 64, 0, 64, 16, 32), "split_halo", (8, 16, 64), None),
        "split halo 4x32x64": ((2, 64, 0, 128, 12, 32), "split_halo", (4, 32, 64), None),
        "split ws 8x16x128": ((2, 128, 0, 128, 16, 16), "split_ws", (8, 16, 128), None),
        "w512": ((cus, 128, 0, 128, 16, 16), "split_w512", (16, 16, 128), 4),
        "p64": ((64, 64, 0, 64, 32, 32), "split_p64", (16, 16, 64), 4),
        "halo 8x32x64": ((2, 64, 0, 64, 16, 32), "halo", (8, 32, 64), None),
        "halo 8x16x64": ((2, 64, 0, 64, 16, 16), "halo", (8, 16, 64), None),
        "halo 4x32x128": ((1, 128, 0, 128, 8, 32), "halo", (4, 32, 128), None),
        "halo 8x16x128": ((2, 128, 0, 128, 16, 16), "halo", (8, 16, 128), None),
    }


CASES_PRO = ["split halo 8x16x64", "split halo 4x32x64", "split ws 8x16x128", "w512", "p64", "halo 8x32x64", "halo 8x16x64", "halo 4x32x128",
             "halo 8x16x128"]


@pytest.mark.parametrize("pro", ("tables", "border"))
@pytest.mark.parametrize("name", CASES_PRO)
def test_conv3x3_prologue(name, pro, cus):
    shape, kernel, tile, distinct = cases_pro(cus)[name]
    d = make_case32(shape, pro="tables", family="border" if pro == "border" else "normal", seed=200 + CASES_PRO.index(name), distinct=distinct)
    check_variants(f"{name} prologue={pro}", d, kernel, tile)


# ------------------------------------------------------------------------------------------------------------------------------
# 1x1
# ------------------------------------------------------------------------------------------------------------------------------
CASES1 = {
    "128x64 ragged": ((8, 64, 64, 64, 6, 6), (128, 64)),               # M = 288 ragged, HW = 36: a tile spans four images
    "128x128": ((2, 128, 64, 128, 16, 16), (128, 128)),
    "out-projection": ((3, 128, 0, 64, 12, 12), (128, 64)),            # attention's out-projection, HW = 144
    "wide K": ((1, 384, 384, 512, 8, 8), (128, 128)),                  # K = 768: three flushes of the split gather kernel
}


@pytest.mark.parametrize("res", (None, "add", "tables"))
@pytest.mark.parametrize("kernel", ("split_igemm", "igemm"))
@pytest.mark.parametrize("name", list(CASES1))
def test_conv1x1_epilogues(name, kernel, res):
    shape, tile = CASES1[name]
    d = make_case32(shape, K=1, res=res, seed=300 + list(CASES1).index(name))
    refs = refs32(d, kernel)
    got = run(d, storage=storage_of(kernel))
    check_one(f"1x1 {name} residual={res}", d, got, kernel, tile, OFF, refs)
    if res:
        inp = run(d, in_place=1, storage=storage_of(kernel))
        assert torch.equal(inp["out"], got["out"]), "the in-place launch differs from the out-of-place one"
        print(f"1x1 {name} [{kernel}] residual={res} in_place=1: bit-identical")


# ------------------------------------------------------------------------------------------------------------------------------
# edges
# ------------------------------------------------------------------------------------------------------------------------------
ZERO = {     # name -> (shape, K, kernel, tile, bit-identical to the single-source call for (x1 = 0, x0 = 0)): the module docstring says why
    "split halo 8x16x64": ((2, 64, 64, 64, 16, 32), 3, "split_halo", (8, 16, 64), (False, False)),
    "split ws 8x16x128": ((2, 64, 64, 128, 16, 16), 3, "split_ws", (8, 16, 128), (False, False)),
    "split gather": ((3, 72, 48, 64, 16, 8), 3, "split_igemm", (128, 64), (False, False)),
    "split 1x1": ((8, 64, 64, 64, 6, 6), 1, "split_igemm", (128, 64), (False, False)),
    "halo 8x32x64": ((2, 64, 64, 64, 16, 32), 3, "halo", (8, 32, 64), (True, True)),
    "gather": ((3, 72, 48, 64, 16, 8), 3, "igemm", (128, 64), (True, False)),
    "1x1": ((8, 64, 64, 64, 6, 6), 1, "igemm", (128, 64), (True, True)),
}


@pytest.mark.parametrize("name", list(ZERO))
def test_zero_sources(name):
    shape, K, kernel, tile, exact = ZERO[name]
    for which, fam in ((0, "zero_x1"), (1, "zero_x0")):
        d = make_case32(shape, K=K, family=fam, seed=400 + which)
        two = run(d, storage=storage_of(kernel))
        refs = refs32(d, kernel)
        check_one(f"zero sources {name} {fam}", d, two, kernel, tile, OFF, refs)
        one = run(single_source(d, which), storage=storage_of(kernel))
        same = torch.equal(two["out"], one["out"])
        core = refs.cores[0][1]
        q = float(((two["out"] - one["out"]).abs() / (2 * core["tol"])).max())
        print(f"zero sources {name} {fam}: against the single-source call, bit-identical {same}, largest difference / (2 tolerance) {q:.3g}")
        if exact[which]:
            assert same, f"{name} {fam}: differs from the single-source call"
        assert q <= 1.0


STRADDLE = {   # name -> (shape, kernel, tile) with 8 groups: 24 channels in 64-channel tiles, 48 in 128-channel ones
    "split halo, 24 channels": ((2, 64, 0, 192, 16, 32), "split_halo", (8, 16, 64)),
    "halo, 24 channels": ((2, 64, 0, 192, 16, 32), "halo", (8, 32, 64)),
    "halo, 48 channels": ((1, 64, 0, 384, 8, 32), "halo", (4, 32, 128)),
}


@pytest.mark.parametrize("name", list(STRADDLE))
def test_groups_that_straddle_a_channel_tile_are_never_fused(name):
    shape, kernel, tile = STRADDLE[name]
    d = make_case32(shape, seed=450 + list(STRADDLE).index(name))
    check_one(name, d, run(d, storage=storage_of(kernel)), kernel, tile, OFF, refs32(d, kernel))    # the conv itself is as good as any
    for storage in (storage_of(kernel), _lib.CF_STORE_BF16):
        with pytest.raises(_lib.PrgError, match="groupnorm: C/VEC must be a power of two"):         # no fused slabs, and no pass either
            run(d, stats=SLABS, storage=storage, want_slabs=True)
    print(f"{name}: statistics are refused in storage {storage_of(kernel)} and in bf16, not made of another tile's channels")


INF_CASES = ["split halo 8x16x64", "split halo 4x32x64 two-source", "split ws 8x16x128 two-source", "split gather fused",
             "split gather separate pass", "halo 8x32x64 two-source", "halo 8x16x128 two-source", "gather fused"]


@pytest.mark.parametrize("name", INF_CASES)
def test_an_infinity_poisons_its_image_only(name, cus):
    d, kernel, tile, _ = case3(name, cus, seed=500 + INF_CASES.index(name))
    d["x0"][1, 5, 3, 4] = float("inf")
    refs = refs32(d, kernel, skip=(1,))
    got = run(d, stats=SLABS, storage=storage_of(kernel), want_slabs=True)
    assert not bool(torch.isfinite(got["sums"][1]).any()), name + ": every group of image 1 reports non-finite sums"
    assert bool(torch.isnan(got["coef_a"][1]).all()) and bool(torch.isnan(got["coef_b"][1]).all()), name + ": NaN coefficients"
    check_one(f"+Inf in image 1, {name}, the other images", d, got, kernel, tile, SLABS, refs)


AMP_CASES = {"split halo 8x16x64": 6, "split halo 4x32x64 two-source": 6, "split ws 8x16x128 two-source": 6, "w512": None, "p64": None,
             "split gather fused": 6, "split gather separate pass": 6, "halo 8x32x64 two-source": 6, "halo 8x16x128 two-source": 6,
             "gather fused": 6}


@pytest.mark.parametrize("family", ("amplitude", "tiny"))
@pytest.mark.parametrize("name", list(AMP_CASES))
def test_amplitudes(name, family, cus):
    """per-image rms 2^-6 .. 2^9 (over the four distinct images of a large batch), and rms 2^-16: every hi half is an f16 subnormal"""
    d, kernel, tile, modes = case3(name, cus, family=family, seed=700 + list(AMP_CASES).index(name), batch=AMP_CASES[name] if family == "amplitude" else None)
    check_variants(f"{family}, {name}", d, kernel, tile, modes)


# ------------------------------------------------------------------------------------------------------------------------------
# the persistent and the one-wave-per-SIMD kernels forced at small shapes, in a process of its own (the switches are read once)
# ------------------------------------------------------------------------------------------------------------------------------
FORCED = [   # (name, shape, kernel, tile, prologue)
    ("p64 grid no multiple of 8, prologue", (3, 64, 0, 64, 48, 32), "split_p64", (16, 16, 64), "tables"),
    ("p64 grid no multiple of 8", (3, 64, 0, 64, 48, 32), "split_p64", (16, 16, 64), None),
    ("p64 several tiles per workgroup, prologue", (5, 128, 0, 64, 16, 48), "split_p64", (16, 16, 64), "tables"),
    ("p64 several tiles per workgroup", (5, 128, 0, 64, 16, 48), "split_p64", (16, 16, 64), None),
    ("w512 two tiles per image, prologue", (2, 128, 0, 128, 32, 16), "split_w512", (16, 16, 128), "tables"),
    ("w512 two tiles per image", (2, 128, 0, 128, 32, 16), "split_w512", (16, 16, 128), None),
    ("w512 two channel tiles, two-source", (1, 64, 64, 256, 16, 32), "split_w512", (16, 16, 128), None),
]


def forced_child():
    """runs in the child: every FORCED case with statistics off and as slabs; prints one JSON line"""
    res = []
    for i, (name, shape, kernel, tile, pro) in enumerate(FORCED):
        d = make_case32(shape, pro=pro, seed=800 + i)
        refs = refs32(d, kernel)
        outs = []
        for stats in (OFF, SLABS):
            got = run(d, stats=stats, storage=storage_of(kernel), want_slabs=True)
            how = "fused" if stats == SLABS and not got["flags"][2] else ("pass" if stats == SLABS else None)
            full = lambda core, g: reference32(d, kernel, tile, stats=how, core=core, from_output=g["out"][core["images"]] if how == "pass" else None)
            worst = {}
            for _, core in refs.cores:
                worst = ratios32(f"forced {name} stats={stats}", got, full(core, got))
            res.append(dict(name=name, stats=stats, choice=list(got["choice"]), flags=list(got["flags"]), ratios=worst))
            outs.append(got["out"])
        res.append(dict(name=name, same_output=bool(torch.equal(outs[0], outs[1]))))
    print("RES " + json.dumps(res))


def test_forced_persistent_and_one_wave_per_simd_kernels():
    """PRG_SPLIT_P64=1 PRG_SPLIT_W512=2 in a fresh process: conv3x3_split_p64_kernel with a grid that is no multiple of 8 and with
    several tiles per workgroup, conv3x3_split_w512_kernel below one tile per CU; prologue + slabs and two-source + slabs, the
    references and tolerances of every other case here"""
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_conv_fused_f32 as m; m.forced_child()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PRG_SPLIT_P64="1", PRG_SPLIT_W512="2"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RES ")][-1][4:])
    by_name = {(e["name"], e.get("stats")): e for e in res}
    for name, shape, kernel, tile, pro in FORCED:
        for stats in (OFF, SLABS):
            e = by_name[(name, stats)]
            choice, flags = expected(kernel, tile, shape, 8, stats)
            print(f"forced {name} [{tname(kernel, tile)}] stats={stats} expect {flags}: largest error / tolerance " +
                  ", ".join(f"{k} {v:.3g}" for k, v in e["ratios"].items()))
            assert tuple(e["choice"]) == choice and tuple(e["flags"]) == flags, e
            assert max(e["ratios"].values()) <= 1.0, e
        assert by_name[(name, None)]["same_output"], name + ": the statistics mode changed the output"
