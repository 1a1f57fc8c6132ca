"""Stochastic DDNM on the device: the keep mask of sampler_step_kernel (csrc/sampler.hip), its Philox uniforms, the keep table of
the sampler handle and GaussianDiffusion.sample / denoise on top of them.  Run with `-m gpu`.

What is compared with what:
  * the mask alone, read out through a row x' = 1 * x0 with u = 0 and a condition depth of 0.75 (kept pixels read 0.75, dropped and
    unknown ones 0), against the raw Philox oracle (oracle/philox.py) under the counter layout of include/prg.h: bit for bit, the
    uniform being an exact 24-bit integer times 2^-24.
  * every row kind with a threshold against the numpy float32 restatement of include/prg.h of tests/test_gpu_sampler_step.py, the keep
    rule stated as "a known pixel that is not kept is an unknown pixel" (except on the refine row, which ignores it): bit for bit.
  * the six reference chains of G23_ddnm_dropout: FP32_TOL = 1e-4, the bound of tests/test_gpu_parity.py and
    tests/test_gpu_sampler_step.py for these short chains on this network; pixels that leave as the condition bit for bit.
  * the seeded path against the stored path fed the oracle's draws: transition k takes keep draw k + 1.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _ddnm_dropout import check_denoise_masks, CHAINS, FP32_TOL, P, diffusion, keep_uniforms, known_mask, last_kept, oracle_keep_draws, oracle_normals, run
from oracle import philox as PH
from pointreggpt_amd import weights as W
from test_gpu_sampler_step import GUARD, ROW_CASES, ROW_SHAPES, SEEDS, draws, hip, reference_a, row_inputs, rows, seeds_for  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4), (3, 144), (64, 16384), (300, 2048)]      # one quad | partial workgroup | four grid strides | B > 256
THRESHOLDS = [0.0, 2.0 ** -24, 0.3, 0.5, 1.0 - 2.0 ** -24, 1.0]
DEPTH = np.float32(0.75)
# x' = 1 * x0: with u = 0 the new state is the condition depth where a known pixel is replaced and 0 elsewhere
MASK_ROW = dict(t=0, clip_pred=0, c_x0=1.0, c_x=0.0, c_eps=0.0, sigma=0.0, sqrt_recip=1.0, sqrt_recipm1=1.0)


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def step_c(hip, row):
    return hip._lib.StepC(int(row["t"]), int(row["clip_pred"]), row["c_x0"], row["c_x"], row["c_eps"], row["sigma"], row["sqrt_recip"],
                          row["sqrt_recipm1"])


def run_step_keep(hip, row, x, u, cond, seeds, keep_p, keep_u=None, reps=1, plain=False):
    """`reps` launches of sampler_step_kernel with the threshold keep_p on host arrays; keep_u (reps,B,HW) stored uniforms or None =
    Philox; plain: through prg_debug_sampler_step (no table at all).  x sits between two guard rows that must come back untouched."""
    B, HW = x.shape
    buf = torch.full((B + 2, HW), GUARD, dtype=torch.float32, device="cuda")
    buf[1:B + 1] = D(np.asarray(x, dtype=np.float32))
    xin = buf[1:B + 1]
    ud = D(np.asarray(u, dtype=np.float32))
    cd = None if cond is None else D(np.asarray(cond, dtype=np.float32))
    sd = D(np.array(seeds, dtype=np.uint64).view(np.int64))
    kd = None if keep_u is None else D(np.asarray(keep_u, dtype=np.float32))
    assert kd is None or tuple(kd.shape) == (reps, B, HW)
    rc = step_c(hip, row)
    L = hip._lib
    if plain:
        L.check(hip.lib.prg_debug_sampler_step(L.ptr(xin), L.ptr(ud), L.ptr(cd), L.ptr(sd), C.byref(rc), B, HW, reps, None, None))
    else:
        L.check(hip.lib.prg_debug_sampler_step_keep(L.ptr(xin), L.ptr(ud), L.ptr(cd), L.ptr(sd), C.byref(rc), float(np.float32(keep_p)),
                                                    L.ptr(kd), B, HW, reps, None, None), "prg_debug_sampler_step_keep")
    out = buf.cpu().numpy()
    assert np.all(out[0] == GUARD) and np.all(out[-1] == GUARD), "sampler_step_kernel wrote outside x"
    return out[1:B + 1].copy()


def mask_cond(B, HW, known):
    cond = np.empty((B, 2, HW), dtype=np.float32)
    cond[:, 0] = DEPTH
    cond[:, 1] = np.where(known, np.float32(1.0), np.float32(-1.0))
    return cond


def read_mask(hip, seeds, HW, draw, p, known=None):
    """The keep mask of Philox draw `draw` (>= 1) under threshold p as booleans (B, HW); every launch overwrites x (c_x = 0)."""
    B = len(seeds)
    known = np.ones((B, HW), dtype=bool) if known is None else known
    z = np.zeros((B, HW), dtype=np.float32)
    got = run_step_keep(hip, MASK_ROW, z, z, mask_cond(B, HW, known), seeds, p, reps=draw)
    assert np.isin(got, [np.float32(0), DEPTH]).all()
    return got == DEPTH


@pytest.fixture(scope="module")
def oracle_u():
    cache = {}

    def get(seed, draw, n, domain=None):
        key = (seed, draw, n, domain)
        if key not in cache:
            cache[key] = keep_uniforms(seed, draw, n) if domain is None else keep_uniforms(seed, draw, n, domain=domain)
        return cache[key]

    return get


# ------------------------------------------------------------------------------------------------------------------
# 1. the keep mask alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW", SHAPES)
def test_keep_mask_is_the_oracles(hip, oracle_u, B, HW):
    seeds = seeds_for(B)
    known = np.random.default_rng(B).random((B, HW)) < 0.75
    known[:, 0] = True
    for draw in (1, 2, 3):
        ref_u = np.stack([oracle_u(s, draw, HW) for s in seeds])
        for p in THRESHOLDS:
            got = read_mask(hip, seeds, HW, draw, p, known)
            ref = known & (ref_u > np.float32(p))
            assert np.array_equal(got, ref), (B, HW, draw, p, int((got != ref).sum()))
            if p == 1.0:
                assert not got.any()                              # u < 1 always: nothing is kept
            if p == 0.0:
                assert np.array_equal(got, known & (ref_u != 0))  # a draw like any other: only u == 0 is dropped


def test_kept_fraction_of_known_pixels(hip):
    """(64, 16384), p = 0.3, 64 DISTINCT keys (the SEEDS list repeats, and equal keys give equal masks): the kept count of the n known
    pixels is Binomial(n, 0.7) up to the 2^-24 grid, so the fraction lies within 6 standard deviations sqrt(p (1 - p) / n) of 0.7."""
    B, HW = 64, 16384
    seeds = [(SEEDS[b % len(SEEDS)] + 0x9E3779B97F4A7C15 * (b + 1)) & (2 ** 64 - 1) for b in range(B)]
    assert len(set(seeds)) == B
    known = np.random.default_rng(64).random((B, HW)) < 0.55
    got = read_mask(hip, seeds, HW, 1, 0.3, known)
    n = int(known.sum())
    frac = float(got.sum()) / n
    bound = 6 * np.sqrt(0.3 * 0.7 / n)
    print(f"kept fraction of {n} known pixels at p = 0.3: {frac:.6f} (0.7 +- {bound:.6f})")
    assert not got[~known].any() and abs(frac - 0.7) <= bound


# ------------------------------------------------------------------------------------------------------------------
# 2. the mask depends on (seed, draw, pixel) only
# ------------------------------------------------------------------------------------------------------------------
def test_keep_mask_depends_on_its_seed_draw_and_pixel_only(hip, oracle_u):
    for B, HW in [(3, 144), (64, 16384), (300, 2048)]:
        seeds = seeds_for(B)
        m1 = read_mask(hip, seeds, HW, 1, 0.3)
        for b in range(len(SEEDS), B):
            assert np.array_equal(m1[b], m1[b % len(SEEDS)]), (B, HW, b)
        for b in range(1, min(B, len(SEEDS))):
            assert not np.array_equal(m1[b], m1[0])
        perm = np.random.default_rng(B).permutation(B)
        assert np.array_equal(read_mask(hip, [seeds[p] for p in perm], HW, 1, 0.3), m1[perm]), (B, HW)
        assert not np.array_equal(read_mask(hip, seeds, HW, 2, 0.3), m1)
        # not the normals' stream: the same counter with the normals' domain word gives another mask
        other = np.stack([oracle_u(s, 1, HW, PH.DOMAIN) for s in seeds]) > np.float32(0.3)
        assert not np.array_equal(m1, other) and float((m1 != other).mean()) > 0.2
    m300 = read_mask(hip, seeds_for(300), 2048, 1, 0.3)
    alone = read_mask(hip, [seeds_for(300)[299]], 2048, 1, 0.3)
    assert np.array_equal(alone[0], m300[299])
    # a prefix of a larger image is the smaller image
    assert np.array_equal(read_mask(hip, seeds_for(64), 16384, 1, 0.3)[0, :2048], m300[0])


# ------------------------------------------------------------------------------------------------------------------
# 3. every row kind with a keep threshold
# ------------------------------------------------------------------------------------------------------------------
def stored_uniforms(B, HW, cond, p, plants):
    """(1, B, HW) uniforms on the 2^-24 grid; the first known pixels of every image hold `plants`."""
    g = np.random.default_rng(7000 + B)
    ku = (g.integers(0, 2 ** 24, (B, HW)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    known = (cond[:, 1] + np.float32(1)) * np.float32(0.5) > np.float32(0.5)
    for b in range(B):
        idx = np.flatnonzero(known[b])[:len(plants)]
        assert len(idx) == len(plants)
        ku[b, idx] = plants
    return ku[None]


def reference_keep(row, x, u, cond, n, p, ku):
    """reference_a (include/prg.h in float32, one rounding per operation) with the keep rule: on a row that draws, a known pixel
    whose uniform is not > p is treated as unknown.  The refine row and a run without a condition ignore the table."""
    if cond is None or int(row["clip_pred"]) & 4 or p < 0:
        return reference_a(row, x, u, cond, n)
    known = (cond[:, 1] + np.float32(1)) * np.float32(0.5) > np.float32(0.5)
    thinned = cond.copy()
    thinned[:, 1] = np.where(known & (ku > np.float32(p)), cond[:, 1], np.float32(-1.0))
    return reference_a(row, x, u, thinned, n)


@pytest.mark.parametrize("name,with_cond", ROW_CASES)
def test_every_row_kind_with_a_threshold(hip, draws, row_inputs, rows, name, with_cond):
    row, kind, _t, _tn = rows[name]
    f = np.float32
    for B, HW in ROW_SHAPES:
        x, u, cond = row_inputs(B, HW)
        n1 = draws(B, HW)[0]
        seeds = seeds_for(B)
        plain = run_step_keep(hip, row, x, u, cond if with_cond else None, seeds, -1.0, plain=True)
        nan_u = np.full((1, B, HW), np.nan, dtype=np.float32)
        off = run_step_keep(hip, row, x, u, cond if with_cond else None, seeds, -1.0, keep_u=nan_u)
        assert np.array_equal(off, plain, equal_nan=True), (name, B, HW)         # keep_p < 0: today's result, the slab unread
        p03 = f(0.3)
        cases = [(p03, [p03, np.nextafter(p03, f(1)), np.nextafter(p03, f(0)), f(0), f(1 - 2.0 ** -24)]),
                 (f(0), [f(0), f(2.0 ** -24), f(1 - 2.0 ** -24)])]
        for p, plants in cases:
            ku = stored_uniforms(B, HW, cond, p, plants)
            got = run_step_keep(hip, row, x, u, cond if with_cond else None, seeds, p, keep_u=ku)
            ref = reference_keep(row, x, u, cond if with_cond else None, n1, p, ku[0])
            assert np.array_equal(got, ref, equal_nan=True), (name, B, HW, float(p), int((got != ref).sum()))
            if kind == "refine" or not with_cond:
                assert np.array_equal(got, plain, equal_nan=True)                # independent of p
            else:
                assert not np.array_equal(got, plain, equal_nan=True)            # the threshold does something
                known = (cond[:, 1] + f(1)) * f(0.5) > f(0.5)
                first = np.array([np.flatnonzero(known[b])[:len(plants)] for b in range(B)])
                kept_planted = np.array(plants) > p                              # u == p and below: dropped; above: kept
                same = np.take_along_axis(got, first, 1) == np.take_along_axis(plain, first, 1)
                assert same[:, kept_planted].all()                               # a kept pixel is the plain DDNM pixel


# ------------------------------------------------------------------------------------------------------------------
# 4. the reference's six chains
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net16(hip, golden):
    net = hip.Unet(16, dtype="fp32").load_state_dict(W.synth_state_dict(W.unet_config(16), 9))
    yield net.set_time_freqs(golden("G0_host_tables")["freqs_dim16"])
    net.close()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", list(CHAINS))
def test_reference_chains_fp32(hip, golden, net16, name, graph):
    g = golden("G23_ddnm_dropout")
    _kw, refine, method = CHAINS[name]
    d = diffusion(hip.GaussianDiffusion, net16, name, golden)
    out = run(d, name, g, D, use_graph=graph).cpu().numpy()
    again = run(d, name, g, D, use_graph=graph).cpu().numpy()
    zeros = run(d, name, g, D, uniforms=np.nan_to_num(g[name + "_uniforms"], nan=0.0), use_graph=graph).cpu().numpy()
    d.close()
    e = float(np.abs(out.astype(np.float64) - g[name + "_out"]).max())
    print(f"{name} graph={graph}: |hip - reference|max = {e:.3e}")
    assert np.isfinite(out).all() and e <= FP32_TOL, (name, e)
    assert np.array_equal(out, again) and np.array_equal(out, zeros)        # replay is exact; the NaN slabs are never read
    if method == "sample" and not refine:
        kept = last_kept(g, name)
        assert kept.any() and np.array_equal(out[kept], g[name + "_out"][kept])


# ------------------------------------------------------------------------------------------------------------------
# 5. the seeded production path
# ------------------------------------------------------------------------------------------------------------------
CHAIN_SEEDS = [SEEDS[3], SEEDS[2]]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", ["T8_linear", "ddim5_none", "denoise_T8", "denoise_ddim5_refine"])
def test_seeded_chain_consumes_keep_draw_k_plus_1(hip, golden, net16, name, graph):
    g = golden("G23_ddnm_dropout")
    _kw, refine, method = CHAINS[name]
    d = diffusion(hip.GaussianDiffusion, net16, name, golden)
    n_rows = len(g[name + "_keep_p"])
    call = getattr(d, method)
    kw = dict(param_cond=D(g["pc"]), img_cond=D(g["cond"]), has_refine_step=refine, use_graph=graph)
    nz = oracle_normals(CHAIN_SEEDS, 0, d.n_draws, 32).cuda()
    seeded = call(seeds=CHAIN_SEEDS, **kw).cpu().numpy()
    stored = call(noise=nz, keep_draws=oracle_keep_draws(CHAIN_SEEDS, 0, n_rows, 32).cuda(), **kw).cpu().numpy()
    half = call(noise=nz, seeds=CHAIN_SEEDS, **kw).cpu().numpy()                       # stored normals, Philox keep mask
    shifted = call(noise=nz, keep_draws=oracle_keep_draws(CHAIN_SEEDS, 1, n_rows, 32).cuda(), **kw).cpu().numpy()
    again = call(seeds=CHAIN_SEEDS, **kw).cpu().numpy()
    if method == "denoise":
        check_denoise_masks(d, refine, oracle_keep_draws(CHAIN_SEEDS, 0, n_rows, 32).numpy(),
                            oracle_keep_draws(CHAIN_SEEDS, 1, n_rows, 32).numpy(), g["cond"], stored, shifted)
    d.close()
    e = float(np.abs(seeded - stored).max())
    known = known_mask(g["cond"])
    moved = float((shifted != stored)[known].mean())
    print(f"{name} graph={graph}: |seeded - stored|max = {e:.3e}; known pixels moved by a shift of one keep draw: {moved:.3f}")
    assert np.isfinite(seeded).all() and e <= FP32_TOL
    assert np.array_equal(half, stored) and np.array_equal(again, seeded)              # the masks are exact, replay is exact
    if method == "sample":
        # p = 0.3 on the last transition: two independent masks disagree on 2 * 0.3 * 0.7 of the known pixels.  (denoise's
        # thresholds are 1 or at most 2^-22: its masks hardly depend on which uniforms they are; check_denoise_masks asserts what holds.)
        assert moved > 0.01


def test_sample_and_denoise_do_not_share_a_graph(hip, golden, net16):
    """sample / denoise / sample ... on ONE object under graph replay: each reproduces its first result bit for bit (separate handles
    per mode), and stored keep draws at a new address are picked up by the captured graph."""
    g = golden("G23_ddnm_dropout")
    kw = dict(param_cond=D(g["pc"]), img_cond=D(g["cond"]), seeds=CHAIN_SEEDS, use_graph=True)
    for ddnm in (True, False):
        d = hip.GaussianDiffusion(net16, image_size=32, timesteps=8, ddnm_sampling_dropout=P, is_ddnm_sampling=ddnm)
        s1, n1 = d.sample(**kw).cpu().numpy(), d.denoise(**kw).cpu().numpy()
        s2, n2 = d.sample(**kw).cpu().numpy(), d.denoise(**kw).cpu().numpy()
        s3 = d.sample(**kw).cpu().numpy()
        assert len(d._samplers) == 2
        assert np.array_equal(s1, s2) and np.array_equal(s1, s3) and np.array_equal(n1, n2)
        assert np.array_equal(s1, n1) == ddnm          # is_ddnm_sampling: denoise IS sample; otherwise sample has no condition at all
        if ddnm:
            nz = oracle_normals(CHAIN_SEEDS, 0, d.n_draws, 32).cuda()
            ka, kb = oracle_keep_draws(CHAIN_SEEDS, 0, 8, 32).cuda(), oracle_keep_draws(CHAIN_SEEDS, 3, 8, 32).cuda()
            skw = dict(param_cond=D(g["pc"]), img_cond=D(g["cond"]), noise=nz, use_graph=True)
            a1 = d.sample(keep_draws=ka, **skw).cpu().numpy()
            b1 = d.sample(keep_draws=kb, **skw).cpu().numpy()
            a2 = d.sample(keep_draws=ka, **skw).cpu().numpy()
            ph = d.sample(seeds=CHAIN_SEEDS, **skw).cpu().numpy()         # back to Philox: a null pointer in the graph
            assert np.array_equal(a1, a2) and not np.array_equal(a1, b1) and np.array_equal(ph, a1)
        d.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. validation, and what Tester inherits
# ------------------------------------------------------------------------------------------------------------------
def test_validation(hip, golden, net16):
    g = golden("G23_ddnm_dropout")
    d = diffusion(hip.GaussianDiffusion, net16, "T8_linear", golden)
    with pytest.raises(hip._lib.PrgError):                                         # row 7 draws: 8 slabs are needed
        run(d, "T8_linear", g, D, uniforms=g["T8_linear_uniforms"][:7])
    out = run(d, "T8_linear", g, D).cpu().numpy()                                  # the handle survives the refusal
    assert float(np.abs(out - g["T8_linear_out"]).max()) <= FP32_TOL
    h = d._sampler(2, False, "sample")
    nine = (C.c_float * 9)(*([0.3] * 9))
    with pytest.raises(hip._lib.PrgError):
        hip._lib.check(hip.lib.prg_sampler_set_keep(h, nine, 9))
    with pytest.raises(hip._lib.PrgError):
        hip._lib.check(hip.lib.prg_sampler_set_keep(h, nine, 7))
    hip._lib.check(hip.lib.prg_sampler_set_keep(h, None, 0))                       # NULL clears: plain DDNM
    cleared = run(d, "T8_linear", g, D).cpu().numpy()
    plain = hip.GaussianDiffusion(net16, image_size=32, timesteps=8)
    ref = plain.sample(param_cond=D(g["pc"]), img_cond=D(g["cond"]), noise=D(g["T8_normals"])).cpu().numpy()
    assert np.array_equal(cleared, ref) and not np.array_equal(cleared, out)
    plain.close()
    d.close()


def test_tester_inherits_reproducibility(hip, tmp_path):
    from pointreggpt_amd.tester import Tester
    net = hip.Unet(8, dtype="fp32").init_synthetic(seed=1)
    strips, files = {}, {}
    for tag, p in (("a", P), ("b", P), ("zero", 0.0)):
        d = hip.GaussianDiffusion(net, image_size=32, timesteps=1000, sampling_timesteps=5, ddnm_sampling_dropout=p)
        np.random.seed(3)
        s = Tester(d, batch_size=2, samples_folder=str(tmp_path / tag), seed=9).sample(2, 2)
        strips[tag] = [x.cpu().numpy() for x in s]
        files[tag] = {f.name: f.read_bytes() for f in sorted((tmp_path / tag).iterdir())}
        d.close()
    net.close()
    a, b, zero = strips["a"], strips["b"], strips["zero"]
    assert len(a) == len(b) == 1 and a[0].shape == (2, 1, 32, 64) and np.isfinite(a[0]).all()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                      # every returned strip
    assert len(files["a"]) >= 2 * 2 * 2 and files["a"] == files["b"]           # and every file written: images, clouds, intrinsics
    assert np.array_equal(a[0][..., :32], zero[0][..., :32]) and not np.array_equal(a[0], zero[0])
