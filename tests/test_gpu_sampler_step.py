"""sampler_step_kernel / sampler_init_kernel (csrc/sampler.hip) and their Philox4x32-10 noise, alone.  Run with `-m gpu`.

What is compared with what:
  * the generator: the device's normals, read out bit for bit through a row that writes 0 * x0 + 1 * n, against the float64
    oracle of oracle/philox.py (pinned by the Random123 vectors in tests/test_philox_oracle.py), never against the C++ twin.
    Bound (derived, not observed): logf, sqrtf and sincosf are documented to <= 1 ulp; with the two float32 roundings of
    -2 * log and r * cos that is about 4 ulp of the Box-Muller radius r; the bound is twice that, 8 * 2^-23 * r_ref per pixel.
    A wrong bit in the upper half of any counter or key word moves a value by O(1).
  * the update arithmetic: every row kind against (A) a numpy float32 evaluation of the formula of include/prg.h in its order,
    one rounding per operation, fed the device's own noise: bit for bit; (B) the torch oracle (oracle/diffusion.py), which
    derives its coefficients from the schedule by itself: FP32_TOL, known pixels of ancestral rows exact.
  * the seeded production path (noise = NULL, device step counter, graph replay) against the stored-noise path fed the
    oracle's draws: transition k consumes draw k + 1, the start image draw 0.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import diffusion as OD
from oracle import philox as PH

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
ULP = 2.0 ** -23
NORMAL_BOUND_ULP = 8.0
SEEDS = [0, 1, 2 ** 32, 0x123456789ABCDEF0, 2 ** 64 - 1]
# (B, HW): one quad | partial workgroup | cap of 4 workgroups per image, four strides | B > 256: one workgroup per image, two
# strides | 64 workgroups
SHAPES = [(1, 4), (3, 144), (64, 16384), (300, 2048), (1, 65536)]
ROW_SHAPES = [(3, 144), (64, 16384)]
GUARD = 7.0


class _Model:
    """What GaussianDiffusion reads of its network when it only builds the transition table."""
    random_or_learned_sinusoidal_cond = False
    channels = out_dim = 1


@pytest.fixture(scope="module")
def hip():
    from pointreggpt_amd import _lib
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.unet import Unet

    class NS:
        pass

    ns = NS()
    ns._lib, ns.lib, ns.GaussianDiffusion, ns.Unet = _lib, _lib.load(), GaussianDiffusion, Unet
    return ns


def seeds_for(B):
    return [SEEDS[b % len(SEEDS)] for b in range(B)]


def run_step(hip, row, x, u, cond, seeds, reps=1):
    """`reps` launches of sampler_step_kernel on host arrays x, u (B,HW), cond (B,2,HW) or None; returns the new x.  x sits between
    two guard rows, which must come back untouched."""
    B, HW = x.shape
    buf = torch.full((B + 2, HW), GUARD, dtype=torch.float32, device="cuda")
    buf[1:B + 1] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    xin = buf[1:B + 1]
    ud = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda()
    cd = None if cond is None else torch.from_numpy(np.ascontiguousarray(cond, dtype=np.float32)).cuda()
    sd = torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)).cuda()
    rc = hip._lib.StepC(int(row["t"]), int(row["clip_pred"]), row["c_x0"], row["c_x"], row["c_eps"], row["sigma"], row["sqrt_recip"],
                        row["sqrt_recipm1"])
    hip._lib.check(hip.lib.prg_debug_sampler_step(hip._lib.ptr(xin), hip._lib.ptr(ud), hip._lib.ptr(cd), hip._lib.ptr(sd), C.byref(rc),
                                                  B, HW, reps, None, None), "prg_debug_sampler_step")
    out = buf.cpu().numpy()
    assert np.all(out[0] == GUARD) and np.all(out[-1] == GUARD), "sampler_step_kernel wrote outside x"
    return out[1:B + 1].copy()


READOUT = dict(t=0, clip_pred=0, c_x0=0.0, c_x=0.0, c_eps=0.0, sigma=1.0, sqrt_recip=1.0, sqrt_recipm1=1.0)   # x' = 0 * x0 + 1 * n


def read_draw(hip, seeds, HW, k):
    """Draw k (k >= 1) of every seed, bit for bit: every launch overwrites x (c_x = 0), launch i adds noise index i + 1."""
    z = np.zeros((len(seeds), HW), dtype=np.float32)
    return run_step(hip, READOUT, z, z, None, seeds, reps=k)


@pytest.fixture(scope="module")
def draws(hip):
    """(B, HW) -> [draw 1, draw 2, draw 3] as the device generates them for seeds_for(B); computed once per shape."""
    cache = {}

    def get(B, HW):
        if (B, HW) not in cache:
            cache[(B, HW)] = [read_draw(hip, seeds_for(B), HW, k) for k in (1, 2, 3)]
        return cache[(B, HW)]

    return get


@pytest.fixture(scope="module")
def oracle_normals():
    cache = {}

    def get(seed, draw, n):
        if (seed, draw, n) not in cache:
            cache[(seed, draw, n)] = PH.normals(seed, draw, n)
        return cache[(seed, draw, n)]

    return get


# ------------------------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW", SHAPES)
def test_philox_normals_against_the_oracle(hip, draws, oracle_normals, B, HW):
    """(a) |n_dev - n_ref| <= 8 * 2^-23 * r_ref on every pixel of draws 1, 2, 3; (b) draws differ pairwise."""
    got = draws(B, HW)
    worst = 0.0
    for k, nd in zip((1, 2, 3), got):
        assert np.isfinite(nd).all()
        for b, s in enumerate(seeds_for(B)):
            n, r = oracle_normals(s, k, HW)
            err = np.abs(nd[b].astype(np.float64) - n)
            nz = r > 0
            worst = max(worst, float(np.max(err[nz] / (ULP * r[nz]))) if nz.any() else 0.0)
            bad = err > NORMAL_BOUND_ULP * ULP * r
            assert not bad.any(), (B, HW, k, b, hex(s), int(bad.sum()), float(np.max(err)))
    print(f"Philox normals ({B}, {HW}): max |n_dev - n_ref| = {worst:.3f} ulp of r (bound {NORMAL_BOUND_ULP:.0f})")
    for i in range(3):
        for j in range(i):
            assert not np.array_equal(got[i], got[j])
            assert not np.array_equal(got[i][0], got[j][0])


def test_philox_image_depends_on_its_seed_only(hip, draws):
    """(b) image b is a function of seeds[b]: equal seeds in different slots give equal bits, a permuted batch gives the permuted
    output, and slot 299 of a 300-image batch equals the same seed alone at B = 1."""
    for B, HW in [(3, 144), (64, 16384), (300, 2048)]:
        n1 = draws(B, HW)[0]
        seeds = seeds_for(B)
        for b in range(len(SEEDS), B):
            assert np.array_equal(n1[b], n1[b % len(SEEDS)]), (B, HW, b)
        for b in range(1, min(B, len(SEEDS))):
            assert not np.array_equal(n1[b], n1[0])
        perm = np.random.default_rng(B).permutation(B)
        got = read_draw(hip, [seeds[p] for p in perm], HW, 1)
        assert np.array_equal(got, n1[perm]), (B, HW)
    alone = read_draw(hip, [seeds_for(300)[299]], 2048, 1)
    assert np.array_equal(alone[0], draws(300, 2048)[0][299])
    # a prefix of a larger image is the smaller image: pixel 4q + i depends on (seed, draw, q, i) only
    assert np.array_equal(draws(1, 65536)[0][0, :4], draws(1, 4)[0][0])
    assert np.array_equal(draws(64, 16384)[1][0, :2048], draws(300, 2048)[1][0])


@pytest.mark.parametrize("B,HW", [(64, 16384), (300, 2048)])
def test_step_counter_advances_once_per_launch(hip, draws, B, HW):
    """(c) the last-arriver ticket: with c_x = 1, sigma = 1 three launches from x = 0 leave ((0 + n1) + n2) + n3 in float32."""
    row = dict(READOUT, c_x=1.0)
    z = np.zeros((B, HW), dtype=np.float32)
    got = run_step(hip, row, z, z, None, seeds_for(B), reps=3)
    n1, n2, n3 = draws(B, HW)
    assert np.array_equal(got, ((z + n1) + n2) + n3)


# ------------------------------------------------------------------------------------------------------------------
# the update arithmetic, one row kind at a time
# ------------------------------------------------------------------------------------------------------------------
def production_rows(hip):
    """name -> (row, kind, t, t_next) from the tables the product builds (GaussianDiffusion.step_table / _steps_c)."""
    anc = hip.GaussianDiffusion(_Model(), image_size=32, timesteps=1000)
    ddim = hip.GaussianDiffusion(_Model(), image_size=32, timesteps=1000, sampling_timesteps=5)
    ta, td = anc.step_table(), ddim.step_table()
    pairs = OD.ddim_time_pairs(1000, 5)
    assert [r["t"] for r in td] == [p[0] for p in pairs] and [r["t"] for r in ta[:2]] == [999, 998]
    arr, n = ddim._steps_c(True)
    ref = {f: getattr(arr[n - 1], f) for f, _ in hip._lib.StepC._fields_}
    assert ref["clip_pred"] == 4 and n == 6
    rows = {f"ancestral_t{t}": (ta[999 - t], "ancestral", t, None) for t in (999, 500, 1, 0)}
    for name, i in (("ddim_first", 0), ("ddim_middle", 2), ("ddim_last", 4)):
        rows[name] = (td[i], "ddim", pairs[i][0], pairs[i][1])
    rows["refine"] = (ref, "refine", 0, None)
    assert ta[0]["sigma"] != 0 and ta[999]["sigma"] == 0 and td[2]["c_eps"] != 0 and td[2]["sigma"] != 0
    assert (td[4]["c_x0"], td[4]["c_x"], td[4]["c_eps"], td[4]["sigma"]) == (1.0, 0.0, 0.0, 0.0)
    return rows


ROW_CASES = [("ancestral_t999", True), ("ancestral_t500", True), ("ancestral_t1", True), ("ancestral_t0", True), ("ddim_first", True),
             ("ddim_middle", True), ("ddim_last", True), ("refine", True), ("ddim_middle", False), ("ancestral_t500", False)]


def clamp_np(v):
    return np.clip(v, np.float32(-1.0), np.float32(1.0))        # propagates NaN, like torch.clamp


def reference_a(row, x, u, cond, n):
    """include/prg.h, prg_step, in float32 with one rounding per operation (separate multiply and add), in that order; terms
    whose coefficient is zero are not added, as the kernel skips them."""
    f = np.float32
    x, u, n = x.astype(f), u.astype(f), n.astype(f)
    clip = int(row["clip_pred"])
    x0p = clamp_np(u) if clip & 1 else u
    if cond is not None:
        known = (cond[:, 1] + f(1.0)) * f(0.5) > f(0.5)
        x0 = np.where(known, cond[:, 0], x0p)
    else:
        known = np.zeros(x.shape, dtype=bool)
        x0 = x0p
    if clip & 2:
        x0 = clamp_np(x0)
    if clip & 4:
        return np.where(known, clamp_np(u), x)
    v = f(row["c_x0"]) * x0
    if f(row["c_x"]) != 0:
        v = v + f(row["c_x"]) * x
    if f(row["c_eps"]) != 0:
        eps = (f(row["sqrt_recip"]) * x - x0p) / f(row["sqrt_recipm1"])
        v = v + f(row["c_eps"]) * eps
    if f(row["sigma"]) != 0:
        v = v + f(row["sigma"]) * n
    assert v.dtype == np.float32
    return v


def reference_b(sch, kind, t, tn, x, u, cond, n):
    """The same transition by the torch oracle, the network replaced by `u`; coefficients from the oracle's own schedule."""
    B, HW = x.shape
    S = int(round(HW ** 0.5))
    T4 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).reshape(B, -1, S, S)
    xt, ut, nt = T4(x), T4(u), T4(n)
    ct = None if cond is None else T4(cond)
    den = lambda *_: ut
    if kind == "ancestral":
        out, _ = OD.p_sample(sch, den, xt, t, None, ct, nt if t > 0 else None)
    elif kind == "refine":
        out = OD.refine(sch, den, xt, None, ct)
    else:                                                    # one pair of ddim_sample (oracle/diffusion.py), eta = 1
        eps, x0 = OD.model_predictions(sch, den, xt, t, None, ct, clip_x_start=True)
        if tn < 0:
            out = x0
        else:
            a, an = sch["alphas_cumprod"][t], sch["alphas_cumprod"][tn]
            sigma = 1.0 * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
            c = (1 - an - sigma ** 2).sqrt()
            out = x0 * an.sqrt() + c * eps + sigma * nt
    return out.reshape(B, HW).numpy()


@pytest.fixture(scope="module")
def row_inputs():
    """(B, HW) -> x, u, cond: u beyond +-1 on both sides (the clamp is active and idle), condition depth in +-1.5 (ancestral rows
    clamp it after the replacement, DDIM rows do not), mask channel over {-1, 1, 0, 1e-7, -1e-7}: (m + 1) * 0.5 > 0.5 is false, true,
    false, true, false."""
    cache = {}

    def get(B, HW):
        if (B, HW) not in cache:
            g = np.random.default_rng(1000 + B)
            x = g.standard_normal((B, HW)).astype(np.float32)
            u = g.uniform(-3, 3, (B, HW)).astype(np.float32)
            cond = np.empty((B, 2, HW), dtype=np.float32)
            cond[:, 0] = g.uniform(-1.5, 1.5, (B, HW))
            cond[:, 1] = np.array([-1.0, 1.0, 0.0, 1e-7, -1e-7], dtype=np.float32)[g.integers(0, 5, (B, HW))]
            known = (cond[:, 1] + np.float32(1)) * np.float32(0.5) > np.float32(0.5)
            assert np.array_equal(known, np.isin(cond[:, 1], np.array([1.0, 1e-7], dtype=np.float32)))
            for sel in (known, ~known):
                assert (np.abs(u[sel]) > 1).any() and (np.abs(u[sel]) < 1).any() and (np.abs(cond[:, 0][sel]) > 1).any()
            cache[(B, HW)] = (x, u, cond)
        return cache[(B, HW)]

    return get


@pytest.fixture(scope="module")
def rows(hip):
    return production_rows(hip)


@pytest.fixture(scope="module")
def sch():
    return OD.schedule(1000)


def nan_maxerr(a, b):
    assert np.array_equal(np.isnan(a), np.isnan(b))
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    d = d[~np.isnan(a)]
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("name,with_cond", ROW_CASES)
def test_every_row_kind_alone(hip, draws, row_inputs, rows, sch, name, with_cond):
    row, kind, t, tn = rows[name]
    for B, HW in ROW_SHAPES:
        x, u, cond = row_inputs(B, HW)
        cond = cond if with_cond else None
        n1 = draws(B, HW)[0]
        got = run_step(hip, row, x, u, cond, seeds_for(B))
        ref = reference_a(row, x, u, cond, n1)
        assert np.array_equal(got, ref, equal_nan=True), (name, B, HW, int((got != ref).sum()), float(np.abs(got - ref).max()))
        refb = reference_b(sch, kind, t, tn, x, u, cond, n1)
        e = nan_maxerr(got, refb)
        print(f"{name} cond={with_cond} ({B}, {HW}): |hip - oracle|max = {e:.3e}")
        assert e <= FP32_TOL, (name, B, HW, e)
        if kind == "ancestral" and with_cond:
            known = (cond[:, 1] + np.float32(1)) * np.float32(0.5) > np.float32(0.5)
            assert known.any() and np.array_equal(got[known], refb[known])


@pytest.mark.parametrize("name", ["ancestral_t500", "ddim_middle", "refine"])
def test_nonfinite_network_output_stays_visible(hip, draws, row_inputs, rows, sch, name):
    """NaN and +-Inf in the network output, at a known and at an in-painted pixel of every image: clamp is torch.clamp, so Inf
    becomes +-1 and NaN stays NaN (it must not leave the sampler as depth 0); every other pixel is what the clean run gives."""
    row, kind, t, tn = rows[name]
    for B, HW in ROW_SHAPES:
        x, u, cond = row_inputs(B, HW)
        n1 = draws(B, HW)[0]
        known = (cond[:, 1] + np.float32(1)) * np.float32(0.5) > np.float32(0.5)
        bad = u.copy()
        poison = np.zeros((B, HW), dtype=bool)
        spots = {}
        for b in range(B):
            ik, iu = np.flatnonzero(known[b])[:3], np.flatnonzero(~known[b])[:3]
            assert len(ik) == 3 and len(iu) == 3
            for idx in (ik, iu):
                bad[b, idx] = [np.nan, np.inf, -np.inf]
                poison[b, idx] = True
            spots[b] = (ik, iu)
        clean = run_step(hip, row, x, u, cond, seeds_for(B))
        got = run_step(hip, row, x, bad, cond, seeds_for(B))
        ref = reference_a(row, x, bad, cond, n1)
        refb = reference_b(sch, kind, t, tn, x, bad, cond, n1)
        assert nan_maxerr(ref, refb) <= FP32_TOL                 # the two references agree first, NaN positions included
        for b in range(B):
            ik, iu = spots[b]
            if kind == "refine":                                 # known pixels take clamp(u); in-painted ones keep x
                assert np.isnan(ref[b, ik[0]]) and ref[b, ik[1]] == 1.0 and ref[b, ik[2]] == -1.0
                assert np.array_equal(ref[b, iu], x[b, iu])
            else:                                                # in-painted pixels take clamp(u)
                assert np.isnan(ref[b, iu[0]]) and np.isfinite(ref[b, iu[1:]]).all()
        assert np.array_equal(got, ref, equal_nan=True), (name, B, HW, int(((got != ref) & ~(np.isnan(got) & np.isnan(ref))).sum()),
                                                           int(np.isnan(got).sum()), int(np.isnan(ref).sum()))
        assert np.array_equal(got[~poison], clean[~poison]) and np.isfinite(clean).all()


# ------------------------------------------------------------------------------------------------------------------
# the seeded production path
# ------------------------------------------------------------------------------------------------------------------
CHAIN_SEEDS = [SEEDS[3], SEEDS[2], SEEDS[4]]


@pytest.fixture(scope="module")
def chain_setup(hip):
    S, B = 32, 3
    net = hip.Unet(8, dtype="fp32").init_synthetic(seed=1)
    g = torch.Generator().manual_seed(11)
    pc = torch.tensor([[37.9, 38.0, 16.25, 16.0]] * B) + torch.randn((B, 4), generator=g) * 0.3
    cond = torch.cat([torch.rand((B, 1, S, S), generator=g) * 2 - 1, (torch.rand((B, 1, S, S), generator=g) > 0.5).float() * 2 - 1], 1)
    yield net, pc.cuda(), cond.cuda(), S, B
    net.close()


def stored_draws(first, count, S):
    """(count, B, 1, S, S): slab k = float32(oracle draw first + k) of every chain seed."""
    return torch.from_numpy(np.stack([np.stack([PH.normals(s, first + k, S * S)[0].astype(np.float32).reshape(1, S, S) for s in CHAIN_SEEDS])
                                      for k in range(count)]))


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("table", ["ancestral8", "ddim5"])
def test_seeded_chain_consumes_draw_k_plus_1(hip, chain_setup, table, graph):
    """sample(seeds=s) = sample(noise=the oracle's draws 0 .. n-1 of s): the start image is draw 0 and transition k adds draw k + 1,
    through the device step counter, eagerly and under graph replay.  The stored draws are the float32-rounded exact normals, the
    device's are within 8 ulp of them, so the two chains differ by float32 roundoff only; shifted by one draw they are unrelated."""
    net, pc, cond, S, B = chain_setup
    kw = dict(timesteps=8) if table == "ancestral8" else dict(timesteps=1000, sampling_timesteps=5)
    d = hip.GaussianDiffusion(net, image_size=S, **kw)
    assert d.n_draws == (8 if table == "ancestral8" else 5)
    seeded = d.sample(param_cond=pc, img_cond=cond, seeds=CHAIN_SEEDS, use_graph=graph).cpu().numpy()
    stored = d.sample(param_cond=pc, img_cond=cond, noise=stored_draws(0, d.n_draws, S).cuda(), use_graph=graph).cpu().numpy()
    shifted = d.sample(param_cond=pc, img_cond=cond, noise=stored_draws(1, d.n_draws, S).cuda(), use_graph=graph).cpu().numpy()
    again = d.sample(param_cond=pc, img_cond=cond, seeds=CHAIN_SEEDS, use_graph=graph).cpu().numpy()
    d.close()
    known = ((cond[:, 1:2] + 1) * 0.5 > 0.5).cpu().numpy()
    e, e_shift = float(np.abs(seeded - stored).max()), float(np.abs(seeded - shifted)[~known].max())
    print(f"{table} graph={graph}: |seeded - stored|max = {e:.3e}; against draws shifted by one: {e_shift:.3e}")
    assert np.isfinite(seeded).all() and np.array_equal(seeded, again)
    assert e <= FP32_TOL
    assert np.array_equal(seeded[known], stored[known]) and known.any() and (~known).any()
    assert e_shift > 1000 * FP32_TOL


def test_seeded_start_image_is_draw_0(hip, chain_setup):
    """sampler_init_kernel alone, through the identity transition: out = (draw 0 + 1) / 2.  The bound of the generator test, pushed
    through the monotone float32 map x -> (x + 1) * 0.5 (oracle/philox.py, start_image_interval)."""
    net, _pc, _cond, S, _B = chain_setup
    d = hip.GaussianDiffusion(net, image_size=S, timesteps=1000, sampling_timesteps=1)
    rows = d.step_table()[:1]
    rows[0].update(c_x0=0.0, c_x=1.0, c_eps=0.0, sigma=0.0)
    d.step_table = lambda: rows
    pc = torch.tensor([[37.9, 38.0, 16.25, 16.0]] * len(SEEDS), device="cuda")
    out = d.sample(param_cond=pc, seeds=SEEDS).cpu().numpy().reshape(len(SEEDS), -1)
    d.close()
    for b, s in enumerate(SEEDS):
        n, r = PH.normals(s, 0, S * S)
        lo, hi = PH.start_image_interval(n, r, NORMAL_BOUND_ULP)
        assert np.all((out[b] >= lo) & (out[b] <= hi)), (hex(s), int(np.sum((out[b] < lo) | (out[b] > hi))))
        assert np.max(np.abs(out[b] * 2 - 1 - PH.normals(s, 1, S * S)[0])) > 1.0          # not draw 1
