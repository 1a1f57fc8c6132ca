"""One bf16 convolution through launch_conv with the fused options of ConvLaunch (prg_debug_conv_fused) against the float64
references of tests/test_conv_fused_refs.py, whose docstring derives every tolerance used here: two sources, statistics of the
output as slabs and as fixed-point accumulators (and the separate pass when nothing fuses), table and fold prologues, and the 1x1
epilogues (plain, table and fold residual, in place or not).

Every case names the kernel the dispatch of conv.hip is expected to choose and asserts (nsplit, acc_done, stats_pass) against that
kernel's slab formula, so a change of dispatch fails an expectation instead of silently moving the coverage to another kernel.
Launches of 16 images or more are compared with a float64 reference on images {0, 1, B / 2, B - 1} and with a float32 one (t32
doubled) on all of them.  Every case prints its expectation and its largest error / tolerance.

The shape (1, 256, 128, 256, 16, 16), proposed as conv_ws with two channel tiles, has four tiles: launch_ws_cfg2 (conv_ws.hip) declines a launch
with more than one channel tile whose grid is no multiple of 8, so that shape runs on the halo kernel (nsplit 2, no accumulators),
which is what its case here expects; the same conv with B = 4 (16 tiles) is the case that runs conv_ws with two channel tiles.

Observed on an MI355X (256 CUs), largest error / tolerance per family (all 78 cases pass, the module takes 14 - 17 s):
  output      3x3 without prologue: c64 0.96, ws 0.67 .. 0.95, w256 0.89 .. 0.92, halo 0.65 .. 0.87, gather 0.89; with a prologue
              (tables, fold, border): c64 0.94 .. 0.97, ws 0.84 .. 0.96, w256 0.86 .. 0.93, halo 0.92 .. 0.96; 1x1: no residual
              0.988 .. 0.995, add 0.991 .. 0.997, tables 0.989 .. 0.997, fold 0.993 .. 0.997; zero sources 0.83 .. 0.99; amplitudes
              0.89 .. 0.99; the other images beside a +Inf 0.86 .. 0.96; everything beside a poisoned group 0.93 .. 1.00.  The half ulp of
              the bf16 store is the dominant term, and some element of a large output comes close to it.
  sums        fused, slabs and accumulators alike: 5e-6 .. 5e-4 (1.4e-2 on the halo kernel behind a table prologue); the separate
              statistics pass 0.05 .. 0.08.  The bound's leading term is sum t32 = (n + 1) e sum P, the worst case of n float32
              accumulations, four orders of magnitude above what the matrix pipe delivers; the statistics pass has t32 = 0 and sits
              close to its depth e sum |v|.  One slab of 128 left out lands at 34 (tests/test_conv_fused_refs.py).
  coefficients  fused 1.5e-5 .. 3.5e-3 (1.4e-2 halo behind a table prologue), statistics pass 0.04 .. 0.11.
  The gather kernel's zero-x0 call with 72 + 48 channels came out bit-identical to the single-source call although the grouping of
  its products differs; the test only asks for agreement within 2 t32 and a bf16 ulp there.
No case failed at any point: these tests found no defect in the kernels or the dispatch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from pointreggpt_amd import _lib
from test_conv_fused_refs import POISON, conv_reference, half_ulp_bf16, make_case, ratios, reference

pytestmark = pytest.mark.gpu

GUARD = 1024       # float32 guard elements on either side of `out`
OFF, SLABS, ACC = _lib.CF_STATS_OFF, _lib.CF_STATS_SLABS, _lib.CF_STATS_ACC
PRO = {None: _lib.CF_PRO_NONE, "tables": _lib.CF_PRO_TABLES, "fold": _lib.CF_PRO_FOLD}
RES = {None: _lib.CF_RES_NONE, "add": _lib.CF_RES_ADD, "tables": _lib.CF_RES_TABLES, "fold": _lib.CF_RES_FOLD}


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------------------------------------
# the hook
# ------------------------------------------------------------------------------------------------------------------------------
def run(d, stats=OFF, in_place=0, storage=_lib.CF_STORE_BF16, want_slabs=False):
    """one call of the hook.  storage: bf16 (the default) or the float launches of tests/test_gpu_conv_fused_f32.py; want_slabs: the
    raw slabs come back too.  `choice` is the kernel launch_conv reported: (family, th, tw, bm, bn)."""
    lib = _lib.load()
    B, C0, C1, Cout, H, W = d["shape"]
    G = d["groups"]
    keep = []                                    # everything the struct points to stays alive until the call returns

    def dev(t, dtype=torch.float32):
        t = t.to(dtype).contiguous().cuda()
        keep.append(t)
        return t.data_ptr()

    def host(t, dtype=np.float32):
        a = np.ascontiguousarray(t.numpy(), dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    a = _lib.ConvFusedC(B=B, C0=C0, C1=C1, Cout=Cout, H=H, W=W, K=d["K"], groups=G, prologue=PRO[d["pro"]], residual_mode=RES[d["res"]],
                        in_place=in_place, stats=stats, storage=storage)
    a.x0 = dev(d["x0"])
    a.x1 = dev(d["x1"]) if C1 else None
    a.w = host(d["w"])
    a.bias = host(d["bias"]) if d["bias"] is not None else None
    if d["pro"] == "tables":
        a.pro_a, a.pro_b = dev(d["pro_a"]), dev(d["pro_b"])
    if d["res"]:
        a.residual = dev(d["residual"])
    if d["res"] == "tables":
        a.res_a, a.res_b = dev(d["res_a"]), dev(d["res_b"])
    if "fold" in (d["pro"], d["res"]):
        f = d["fold"]
        a.fold_acc, a.fold_p, a.fold_q = dev(f["acc"], torch.int64), host(f["P"]), host(f["Q"])
    n_out = B * Cout * H * W
    big = torch.full((GUARD + n_out + GUARD,), 7.0, dtype=torch.float32, device="cuda")
    a.out = big.data_ptr() + 4 * GUARD
    sums = np.full((B, G, 2), -7.0, dtype=np.float64)
    raw = np.full((B, G, 2), -7, dtype=np.int64)
    coef = torch.full((2, B, Cout), -7.0, dtype=torch.float32, device="cuda")
    if stats != OFF:
        a.gamma, a.beta = host(d["gamma"]), host(d["beta"])
        a.sums, a.coef_a, a.coef_b = sums.ctypes.data, coef[0].data_ptr(), coef[1].data_ptr()
        if stats == ACC:
            a.acc_raw = raw.ctypes.data
    slabs = np.full((B * _lib.CF_MAX_SLABS * G * 2,), -7.0, dtype=np.float32) if want_slabs and stats != OFF else None
    if slabs is not None:
        a.slabs = slabs.ctypes.data
    rc = lib.prg_debug_conv_fused(C.byref(a), _lib.stream_ptr())
    _lib.check(rc, "prg_debug_conv_fused")
    big = big.cpu()
    assert bool((big[:GUARD] == 7.0).all()) and bool((big[GUARD + n_out:] == 7.0).all()), "guard floats were written"
    got = dict(out=big[GUARD:GUARD + n_out].reshape(B, Cout, H, W).double(), flags=(a.nsplit, a.acc_done, a.stats_pass),
               choice=(_lib.CONV_FAMILIES[a.family], a.th, a.tw, a.bm, a.bn))
    if slabs is not None:
        used = B * a.nslabs * G * 2
        assert bool((slabs[used:] == -7.0).all()), "slabs were written past nslabs"
        got["slabs"] = torch.from_numpy(slabs[:used].copy()).reshape(B, a.nslabs, G, 2).double()
    if stats != OFF:
        coef = coef.cpu().double()
        got.update(sums=torch.from_numpy(sums), coef_a=coef[0], coef_b=coef[1], raw=torch.from_numpy(raw))
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# what the dispatch is expected to do
# ------------------------------------------------------------------------------------------------------------------------------
def expected_flags(kernel, tile, shape, groups, stats):
    """(nsplit, acc_done, stats_pass) of `kernel` (with tile (TH, TW, BN), or (BM, BN) for the gather kernel)"""
    if stats == OFF:
        return (0, 0, 0)
    B, C0, C1, Cout, H, W = shape
    cpg = Cout // groups
    if kernel == "igemm":
        ns = (H * W) // tile[0] if (H * W) % tile[0] == 0 else 0           # launch_igemm: HW / BM
        return (ns, 0, 1 if ns == 0 else 0)
    TH, TW, BN = tile
    tiles = (H // TH) * (W // TW)
    if kernel == "c64":
        ns = tiles * 2 * (2 if cpg > 32 else 1)                             # tiles * 2 * split_n
    elif kernel == "ws":
        ns = tiles * (4 // (BN // 64))                                      # tiles * WAVES_M
    elif kernel == "w256":
        ns = tiles * 2
    else:
        ns = tiles                                                          # halo
    return (ns, 1 if stats == ACC and kernel in ("c64", "ws", "w256") else 0, 0)


def stats_kernel(kernel, flags):
    return "gn_stats" if flags[2] else kernel


def chunks(B):
    """float64 on all images of a small batch; on {0, 1, B / 2, B - 1} of a large one, with float32 on all, 16 at a time"""
    if B < 16:
        return [(torch.float64, list(range(B)))]
    return [(torch.float64, sorted({0, 1, B // 2, B - 1}))] + [(torch.float32, list(range(i, min(B, i + 16)))) for i in range(0, B, 16)]


class Refs:
    """conv_reference of one input set, computed once per chunk and shared by the variants that leave the output unchanged"""

    def __init__(self, d, skip=(), conv_ref=conv_reference, chunks_of=chunks):
        self.d = d
        self.cores = [(dt, conv_ref(d, [i for i in im if i not in skip], dt)) for dt, im in chunks_of(d["shape"][0])]

    def check(self, label, got, kernel=None, partials=0, full_ref=None, ratio_fn=ratios):
        """full_ref(core, got) / ratio_fn: another module's reference on a core of its conv_ref, and its comparison"""
        worst = {}
        for dt, core in self.cores:
            idx = core["images"]
            ref = full_ref(core, got) if full_ref else reference(self.d, kernel=kernel, partials=partials, core=core,
                                                                 from_output=got["out"][idx] if kernel == "gn_stats" else None)
            for k, v in ratio_fn(label, got, ref, show=False).items():
                worst[k] = max(worst.get(k, 0.0), v)
        print(f"{label}: largest error / tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, (label, worst)
        return worst


def check_stats_variants(name, d, kernel, tile, refs=None, modes=(OFF, SLABS, ACC), skip=()):
    """the same conv with statistics off, as slabs and with accumulators offered: one output, bit for bit"""
    refs = refs or Refs(d, skip)
    outs = []
    for stats in modes:
        got = run(d, stats=stats)
        want = expected_flags(kernel, tile, d["shape"], d["groups"], stats)
        label = f"{name} [{kernel} {'x'.join(map(str, tile))}] stats={stats} expect (nsplit, acc_done, stats_pass) = {want}"
        assert got["flags"] == want, (label, got["flags"])
        if stats == OFF:
            refs.check(label, got)
        else:
            refs.check(label, got, kernel=stats_kernel(kernel, want), partials=want[0] if want[1] else 0)
            if stats == ACC and not want[1]:
                assert not bool(got["raw"].any()), label + ": declined accumulators must come back zero"
        outs.append(got["out"])
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), name + ": the statistics mode changed the output"
    return refs


# ------------------------------------------------------------------------------------------------------------------------------
# 3x3
# ------------------------------------------------------------------------------------------------------------------------------
def cases3(cus):
    q = cus // 8
    return {
        "c64": ((2, 64, 0, 64, 32, 64), 8, "c64", (8, 32, 64), True),
        "c64 groups=1": ((2, 64, 0, 64, 32, 64), 1, "c64", (8, 32, 64), True),
        "ws 8x32x64": ((2, 64, 0, 64, 16, 32), 8, "ws", (8, 32, 64), True),
        "ws 8x32x64 two-source": ((2, 64, 64, 64, 16, 32), 8, "ws", (8, 32, 64), True),
        "ws 4x32x128": ((1, 128, 64, 128, 8, 32), 8, "ws", (4, 32, 128), True),
        "ws 8x16x128": ((2, 64, 128, 128, 16, 16), 8, "ws", (8, 16, 128), True),
        "four tiles, two channel tiles": ((1, 256, 128, 256, 16, 16), 8, "halo", (8, 16, 128), True),
        "ws two channel tiles": ((4, 256, 128, 256, 16, 16), 8, "ws", (8, 16, 128), True),
        "w256 tw=16": ((cus, 64, 64, 128, 16, 16), 8, "w256", (16, 16, 128), True),
        "w256 tw=32": ((q, 64, 64, 128, 32, 64), 8, "w256", (8, 32, 128), True),
        "halo": ((2, 64, 64, 64, 16, 32), 8, "halo", (8, 32, 64), False),
        "igemm fused": ((3, 72, 48, 64, 16, 8), 8, "igemm", (128, 64), True),
        "igemm unfused": ((3, 72, 48, 64, 12, 12), 8, "igemm", (128, 64), True),
    }


CASES3 = ["c64", "c64 groups=1", "ws 8x32x64", "ws 8x32x64 two-source", "ws 4x32x128", "ws 8x16x128", "four tiles, two channel tiles",
          "ws two channel tiles", "w256 tw=16", "w256 tw=32", "halo", "igemm fused", "igemm unfused"]


@pytest.mark.parametrize("name", CASES3)
def test_conv3x3_sources_and_statistics(name, cus):
    shape, groups, kernel, tile, bias = cases3(cus)[name]
    d = make_case(shape, groups=groups, bias=bias, seed=100 + CASES3.index(name))
    check_stats_variants(name, d, kernel, tile)


# single-source shapes with a prologue: (shape, groups, kernel, tile, bias); the fold on conv_ws and the halo kernel goes through
# launch_gn_coeff_acc (ConvChoice::fill_tables), on conv_c64 and conv_w256 it is folded in the kernel
def cases_pro(cus):
    q = cus // 8
    return {
        "c64": ((2, 64, 0, 64, 32, 64), 8, "c64", (8, 32, 64), True),
        "ws 8x32x64": ((2, 64, 0, 64, 16, 32), 8, "ws", (8, 32, 64), True),
        "ws 4x32x128": ((1, 128, 0, 128, 8, 32), 8, "ws", (4, 32, 128), True),
        "ws 8x16x128": ((2, 128, 0, 128, 16, 16), 8, "ws", (8, 16, 128), True),
        "w256 tw=16": ((cus, 128, 0, 128, 16, 16), 8, "w256", (16, 16, 128), True),
        "w256 tw=32": ((q, 128, 0, 128, 32, 64), 8, "w256", (8, 32, 128), True),
        "halo": ((2, 64, 0, 64, 16, 32), 8, "halo", (8, 32, 64), False),
    }


CASES_PRO = ["c64", "ws 8x32x64", "ws 4x32x128", "ws 8x16x128", "w256 tw=16", "w256 tw=32", "halo"]


@pytest.mark.parametrize("pro", ("tables", "fold", "border"))
@pytest.mark.parametrize("name", CASES_PRO)
def test_conv3x3_prologue(name, pro, cus):
    shape, groups, kernel, tile, bias = cases_pro(cus)[name]
    fam = "border" if pro == "border" else "normal"
    d = make_case(shape, groups=groups, bias=bias, pro="tables" if pro == "border" else pro, family=fam, seed=200 + CASES_PRO.index(name))
    # with statistics as the forward pass asks for them (conv2 of a ResnetBlock): accumulators offered
    check_stats_variants(f"{name} prologue={pro}", d, kernel, tile, modes=(OFF, ACC))


# ------------------------------------------------------------------------------------------------------------------------------
# 1x1
# ------------------------------------------------------------------------------------------------------------------------------
CASES1 = {
    "128x64 ragged": ((8, 64, 64, 64, 6, 6), "igemm 128x64: M = 288 ragged, HW = 36, a tile spans four images"),
    "128x128": ((2, 128, 64, 128, 16, 16), "igemm 128x128"),
    "256x64": ((16, 64, 64, 64, 32, 32), "igemm 256x64"),
    "256x128": ((64, 64, 64, 256, 32, 32), "igemm 256x128"),
    "out-projection": ((3, 128, 0, 64, 12, 12), "igemm 128x64: attention's out-projection, HW = 144"),
}


@pytest.mark.parametrize("res", (None, "add", "tables", "fold"))
@pytest.mark.parametrize("name", list(CASES1))
def test_conv1x1_epilogues(name, res):
    shape, what = CASES1[name]
    d = make_case(shape, K=1, res=res, seed=300 + list(CASES1).index(name))
    refs = Refs(d)
    got = run(d)
    refs.check(f"1x1 {name} [{what}] residual={res}", got)
    if res:
        inp = run(d, in_place=1)
        assert torch.equal(inp["out"], got["out"]), "the in-place launch differs from the out-of-place one"
        print(f"1x1 {name} residual={res} in_place=1: bit-identical")


# ------------------------------------------------------------------------------------------------------------------------------
# edges
# ------------------------------------------------------------------------------------------------------------------------------
def single_source(d, which):
    """the single-source call on x0 (which = 0) or x1 with the matching half of w"""
    B, C0, C1, Cout, H, W = d["shape"]
    s = dict(d)
    s["shape"] = (B, C0 if which == 0 else C1, 0, Cout, H, W)
    s["x0"], s["x1"] = (d["x0"] if which == 0 else d["x1"]), None
    s["w"] = (d["w"][:, :C0] if which == 0 else d["w"][:, C0:]).contiguous()
    return s


ZERO = {     # name -> (shape, K, bias, kernel of the two-source call, kernel of the single-source calls, exact for (x1 = 0, x0 = 0))
    "ws 8x32x64": ((2, 64, 64, 64, 16, 32), 3, True, "ws", "ws", (True, True)),
    "ws 4x32x128": ((1, 128, 64, 128, 8, 32), 3, True, "ws", "ws", (True, True)),
    "halo": ((2, 64, 64, 64, 16, 32), 3, False, "halo", "halo", (True, True)),
    # 72 + 48 channels in chunks of 32: with x0 = 0 the products of x1 start in the middle of a chunk (and of a 16-wide MFMA
    # step), the single-source call's at its start: the same products are added in another grouping, so within t32, not bit for bit
    "igemm": ((3, 72, 48, 64, 16, 8), 3, True, "igemm", "igemm", (True, False)),
    "1x1": ((8, 64, 64, 64, 6, 6), 1, True, "igemm", "igemm", (True, True)),
}


@pytest.mark.parametrize("name", list(ZERO) + ["w256 tw=16"])
def test_zero_sources(name, cus):
    if name == "w256 tw=16":
        shape, K, bias, k2, k1, exact = (cus, 64, 64, 128, 16, 16), 3, True, "w256", "w256", (True, True)
    else:
        shape, K, bias, k2, k1, exact = ZERO[name]
    for which, fam in ((0, "zero_x1"), (1, "zero_x0")):
        d = make_case(shape, K=K, bias=bias, family=fam, seed=400 + which)
        two = run(d)
        refs = Refs(d)
        refs.check(f"zero sources {name} [{k2}] {fam}", two)
        one = run(single_source(d, which))
        if exact[which]:
            assert torch.equal(two["out"], one["out"]), f"{name} {fam}: differs from the single-source call [{k1}]"
            print(f"zero sources {name} {fam}: bit-identical to the single-source call [{k1}]")
        else:
            # both are within t32 of the exact value before the bf16 store: 2 t32 apart, and then a bf16 ulp when they straddle a tie
            core = refs.cores[0][1]
            tol = 2 * core["t32"] + 2 * half_ulp_bf16(core["ref"].abs() + core["t32"])
            q = float(((two["out"] - one["out"]).abs() / tol).max())
            print(f"zero sources {name} {fam}: against the single-source call [{k1}], another grouping of the same products: {q:.3f}")
            assert q <= 1.0


INF_CASES = ["c64", "ws 8x32x64 two-source", "w256 tw=16", "halo", "igemm fused", "igemm unfused"]


@pytest.mark.parametrize("name", INF_CASES)
def test_an_infinity_poisons_its_image_only(name, cus):
    shape, groups, kernel, tile, bias = cases3(cus)[name]
    d = make_case(shape, groups=groups, bias=bias, seed=500 + INF_CASES.index(name))
    d["x0"][1, 5, 3, 4] = float("inf")
    refs = Refs(d, skip=(1,))
    for stats in (SLABS, ACC):
        got = run(d, stats=stats)
        want = expected_flags(kernel, tile, shape, groups, stats)
        label = f"+Inf in image 1, {name} [{kernel}] stats={stats} expect {want}"
        assert got["flags"] == want, (label, got["flags"])
        if want[1]:
            assert bool((got["raw"][1, :, 1] < 0).all()), label + ": the poison bit of every group of image 1"
            assert bool((got["raw"][[0, 2] if shape[0] > 2 else [0], :, 1] >= 0).all())
        else:
            assert not bool(torch.isfinite(got["sums"][1]).any()), label + ": every group of image 1 reports non-finite sums"
        assert bool(torch.isnan(got["coef_a"][1]).all()) and bool(torch.isnan(got["coef_b"][1]).all()), label + ": NaN coefficients"
        refs.check(label + ", the other images", got, kernel=stats_kernel(kernel, want), partials=want[0] if want[1] else 0)


POISON_CASES = {"c64": "pro", "ws 8x32x64": "pro", "w256 tw=16": "pro", "1x1 128x64 ragged": "res", "1x1 256x64": "res"}


@pytest.mark.parametrize("name", list(POISON_CASES))
def test_a_poisoned_accumulator_gives_nan(name, cus):
    if POISON_CASES[name] == "pro":
        shape, groups, kernel, tile, bias = cases_pro(cus)[name]
        d = make_case(shape, groups=groups, pro="fold", seed=600, poison=(1, 3))
        want_nan = torch.zeros(shape[0], shape[3], dtype=torch.bool)
        want_nan[1] = True                                        # every output of the image sums over the poisoned channels
    else:
        shape = CASES1[name[4:]][0]
        d = make_case(shape, K=1, res="fold", seed=601, poison=(1, 3))
        cpg = shape[3] // 8
        want_nan = torch.zeros(shape[0], shape[3], dtype=torch.bool)
        want_nan[1, 3 * cpg:4 * cpg] = True                       # that group's channels only
    assert int(d["fold"]["acc"][1, 3, 1]) < 0 and int(d["fold"]["acc"][1, 3, 1]) & ~POISON > 0
    got = run(d)
    nan = torch.isnan(got["out"])
    assert bool((nan == want_nan[:, :, None, None]).all()), name + ": NaN exactly where the poisoned group reaches"
    Refs(d).check(f"poisoned (image 1, group 3), {name}: everything else", got)


AMP_CASES = {"c64": 6, "ws 8x32x64 two-source": 6, "ws 8x16x128": 6, "w256 tw=32": None, "halo": 6, "igemm fused": 6, "igemm unfused": 6}


@pytest.mark.parametrize("name", list(AMP_CASES))
def test_amplitudes(name, cus):
    shape, groups, kernel, tile, bias = cases3(cus)[name]
    if AMP_CASES[name]:
        shape = (AMP_CASES[name],) + shape[1:]
    d = make_case(shape, groups=groups, bias=bias, family="amplitude", seed=700 + list(AMP_CASES).index(name))
    check_stats_variants(f"rms 2^-6 .. 2^9, {name}", d, kernel, tile, modes=(SLABS, ACC))
