"""objective = pred_noise / pred_v and beta_schedule = linear / cosine without a GPU: the host schedules and tables against the
reference's own arrays (G24_objectives), the C++ twin (prg_cpu_sampler_run_objective) against a numpy float32 restatement of
include/prg.h on single rows, and against every reference chain of the fixture.

Tolerances: schedules and buffers bit for bit (float64 and float32); single rows bit for bit; chains <= FP32_TOL = 1e-4, the bound
of the G9_G10 / G18 / G23 chains on this network, with the pixels that leave the sampler as the condition bit for bit.  The
fixture's own 8-thread and 1-thread outputs lie within FP32_TOL / 4 of each other (asserted when it was generated, and here)."""
import ctypes as C

import numpy as np
import pytest
import torch

from _objectives import BUFFERS, CHAINS, FP32_TOL, OBJECTIVES, SCHEDULES, FakeNet, anc_T, check_chain, diffusion, reference_step, \
    row_kinds, rows_of, run
from pointreggpt_amd import _lib, cpu
from pointreggpt_amd import diffusion as DF
from pointreggpt_amd import weights as W
from pointreggpt_amd.diffusion import GaussianDiffusion

T = torch.tensor
FIXTURE = "G24_objectives"


@pytest.fixture(scope="module")
def net16(golden):
    net = cpu.Unet(16).load_state_dict(W.synth_state_dict(W.unet_config(16), 9))
    yield net.set_time_freqs(golden("G0_host_tables")["freqs_dim16"])
    net.close()


# ------------------------------------------------------------------------------------------------------------------
# 1. schedules and tables
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_schedules_are_the_references_bit_for_bit(golden, schedule):
    g = golden(FIXTURE)
    fn = dict(sigmoid=DF.sigmoid_beta_schedule, cosine=DF.cosine_beta_schedule, linear=DF.linear_beta_schedule)[schedule]
    for steps in (1000, anc_T(schedule)):
        pre = f"{schedule}_T{steps}_"
        betas = fn(steps)
        assert betas.dtype == torch.float64 and g[pre + "betas"].dtype == np.float64
        assert np.array_equal(betas.numpy(), g[pre + "betas"])
        assert np.array_equal(torch.cumprod(1.0 - betas, dim=0).numpy(), g[pre + "alphas_cumprod"])
        buf = DF.make_schedule(steps, schedule)
        assert np.array_equal(buf["betas"].numpy(), g[pre + "betas"].astype(np.float32))
        assert np.array_equal(buf["alphas_cumprod"].numpy(), g[pre + "alphas_cumprod"].astype(np.float32))
        for name in BUFFERS:
            assert buf[name].dtype == torch.float32 and g[pre + name].dtype == np.float32
            assert np.array_equal(buf[name].numpy(), g[pre + name]), (schedule, steps, name)
        # the ancestral refine row takes the posterior mean at t = 0 to be x0 itself
        assert float(buf["posterior_mean_coef1"][0]) == 1.0 and float(buf["posterior_mean_coef2"][0]) == 0.0
        assert g[pre + "posterior_mean_coef1"][0] == 1.0 and g[pre + "posterior_mean_coef2"][0] == 0.0
    if schedule == "cosine":
        assert float(fn(1000).max()) == 0.999                   # clipped
    assert np.array_equal(DF.make_schedule(8)["betas"].numpy(), DF.make_schedule(8, "sigmoid")["betas"].numpy())


def test_rejections_and_nothing_else():
    for steps in (2, 8, 20):                                  # the last beta is 0.02 * 1000 / T >= 1: the reference samples NaN
        with pytest.raises(ValueError):
            DF.make_schedule(steps, "linear")
        with pytest.raises(ValueError):
            GaussianDiffusion(FakeNet(), image_size=32, timesteps=steps, objective="pred_x0", beta_schedule="linear")
    with pytest.raises(ValueError):
        DF.make_schedule(1000, "quadratic")
    for bad in (dict(objective="pred_eps", beta_schedule="cosine"), dict(objective="", beta_schedule="sigmoid"),
                dict(objective="pred_v", beta_schedule="quadratic"), dict(objective="pred_x0", beta_schedule="Cosine"),
                # a configuration other than the generator's names both keywords: the reference's defaults for the one left out
                # (pred_noise / cosine) are not this project's (pred_x0 / sigmoid)
                dict(objective="pred_noise"), dict(objective="pred_v"), dict(beta_schedule="cosine"), dict(beta_schedule="linear"),
                dict(objective="pred_eps"), dict(beta_schedule="quadratic")):
        with pytest.raises(ValueError):
            GaussianDiffusion(FakeNet(), image_size=32, **bad)
        with pytest.raises(ValueError):
            cpu.GaussianDiffusion(FakeNet(), image_size=32, **bad)
    for o in OBJECTIVES:
        for s in SCHEDULES:
            for steps in (21, 40, 1000) + ((8,) if s != "linear" else ()):
                for cls in (GaussianDiffusion, cpu.GaussianDiffusion):
                    d = cls(FakeNet(), image_size=32, timesteps=steps, objective=o, beta_schedule=s)
                    assert (d.objective, d.beta_schedule) == (o, s)
                    assert all(np.isfinite(list(r.values())).all() for r in d.step_table())
    for kw in ({}, dict(objective="pred_x0"), dict(beta_schedule="sigmoid")):      # this project's defaults stay the generator's
        d = GaussianDiffusion(FakeNet(), image_size=32, **kw)
        assert (d.objective, d.beta_schedule) == ("pred_x0", "sigmoid")


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("objective", list(OBJECTIVES))
def test_objective_table(objective, schedule):
    for kw in (dict(timesteps=anc_T(schedule)), dict(timesteps=1000, sampling_timesteps=5)):
        d = GaussianDiffusion(FakeNet(), image_size=32, objective=objective, beta_schedule=schedule, **kw)
        x0 = GaussianDiffusion(FakeNet(), image_size=32, objective="pred_x0", beta_schedule=schedule, **kw)
        for refine in (False, True):
            a, n = d._steps_c(refine)
            b, m = x0._steps_c(refine)
            assert n == m and bytes(a) == bytes(b)             # the transition table does not depend on the objective
            tab = d.objective_table(refine)
            code, cp, cq = d._objective_c(refine)
            assert code == OBJECTIVES[objective]
            if objective == "pred_x0":
                assert tab is None and cp is None and cq is None
                continue
            ts = [a[i].t for i in range(n)]
            assert len(tab) == n and (not refine or ts[-1] == 0)
            bp, bq = ((d.sqrt_recip_alphas_cumprod, d.sqrt_recipm1_alphas_cumprod) if objective == "pred_noise" else
                      (d.sqrt_alphas_cumprod, d.sqrt_one_minus_alphas_cumprod))
            assert [p for p, _ in tab] == [float(bp[t]) for t in ts] and [q for _, q in tab] == [float(bq[t]) for t in ts]
            assert list(cp) == [p for p, _ in tab] and list(cq) == [q for _, q in tab]
            assert all(q > 0 and np.isfinite(p) for p, q in tab)
            if objective == "pred_noise":                      # the same two numbers the row already carries
                assert [(a[i].sqrt_recip, a[i].sqrt_recipm1) for i in range(n)] == tab


# ------------------------------------------------------------------------------------------------------------------
# 2. the twin, one row at a time, against include/prg.h in numpy
# ------------------------------------------------------------------------------------------------------------------
def step_c(row):
    return _lib.StepC(int(row["t"]), int(row["clip_pred"]), row["c_x0"], row["c_x"], row["c_eps"], row["sigma"], row["sqrt_recip"],
                      row["sqrt_recipm1"])


def twin_one_row(net, row, code, x, n1, pc, cond, keep_p=None, ku=None):
    """prg_cpu_sampler_run_objective with the one-row table [row]: start image x, noise slab n1; returns its output (B,HW)."""
    B, HW = x.shape
    S = int(round(HW ** 0.5))
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    noise = f32(np.stack([x, n1]))
    arr = (_lib.StepC * 1)(step_c(row))
    p, q, kp, kua, pcn, cn = f32([row["p"]]), f32([row["q"]]), f32(None if keep_p is None else [keep_p]), f32(ku), f32(pc), f32(cond)
    out = np.empty((B, HW), dtype=np.float32)
    cpu.check(cpu.load().prg_cpu_sampler_run_objective(net.handle, arr, 1, ptr(pcn), ptr(cn), ptr(noise), 2, None, ptr(kp), ptr(kua),
                                                       0 if ku is None else 1, code, ptr(p) if code else None, ptr(q) if code else None,
                                                       ptr(out), B, S), "prg_cpu_sampler_run_objective")
    return out


@pytest.fixture(scope="module")
def row_inputs(golden, net16):
    """x (scaled so that x0r leaves [-1, 1] on a good share of the pixels), a noise slab, the G24 condition, stored uniforms on the
    2^-24 grid, and the network's own output per timestep (the same call the twin makes)."""
    g = golden(FIXTURE)
    rng = np.random.default_rng(24)
    B, HW = 2, 32 * 32
    x = (rng.standard_normal((B, HW)) * 1.5).astype(np.float32)
    n1 = rng.standard_normal((B, HW)).astype(np.float32)
    ku = (rng.integers(0, 2 ** 24, (B, HW)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    cond = g["cond"].reshape(B, 2, HW)
    cache = {}

    def u_of(t):
        if t not in cache:
            cache[t] = net16(T(x.reshape(B, 1, 32, 32)), torch.full((B,), t, dtype=torch.int64), T(g["pc"])).numpy().reshape(B, HW)
        return cache[t]

    return x, n1, ku, cond, g["pc"], u_of


@pytest.mark.parametrize("kind", ["ancestral", "ancestral_t0", "ddim", "ddim_last", "refine"])
@pytest.mark.parametrize("objective", list(OBJECTIVES))
def test_twin_rows_match_the_restatement(net16, row_inputs, objective, kind):
    x, n1, ku, cond, pc, u_of = row_inputs
    code = OBJECTIVES[objective]
    row = row_kinds(GaussianDiffusion, objective)[kind]
    u = u_of(row["t"])
    half = lambda v: (v + np.float32(1.0)) * np.float32(0.5)
    seen = []
    for c in (cond, None):
        for keep_p in (None, 0.3):
            got = twin_one_row(net16, row, code, x, n1, pc, c, keep_p, ku[None] if keep_p is not None else None)
            ref = half(reference_step(row, x, u, c, n1, code, row["p"], row["q"], -1.0 if keep_p is None else keep_p, ku))
            assert np.array_equal(got, ref), (objective, kind, c is None, keep_p, int((got != ref).sum()))
            seen.append(got)
    assert np.array_equal(seen[0], seen[1]) == (kind == "refine")           # the threshold does something, except on the refine row
    assert np.array_equal(seen[2], seen[3])                                 # and nothing without a condition
    if code:                                                                # and the objective does something
        plain = twin_one_row(net16, row, 0, x, n1, pc, cond)
        assert not np.array_equal(plain, seen[0])
        x0r = np.float32(row["p"]) * x - np.float32(row["q"]) * u
        assert 0.05 < float((np.abs(x0r) > 1).mean()) < 0.95                # the clamp is active and idle


def test_twin_rejects_bad_objectives(net16, row_inputs):
    x, n1, _ku, cond, pc, _u = row_inputs
    row = row_kinds(GaussianDiffusion, "pred_v")["ddim"]
    for code in (-1, 3):
        with pytest.raises(_lib.PrgError):
            twin_one_row(net16, row, code, x, n1, pc, cond)
    lib = cpu.load()
    arr = (_lib.StepC * 1)(step_c(row))
    out = np.empty_like(x)
    one = np.ones(1, dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    noise = np.ascontiguousarray(np.stack([x, n1]))
    pcn = np.ascontiguousarray(pc, dtype=np.float32)
    for p, q in ((None, ptr(one)), (ptr(one), None), (None, None)):
        assert lib.prg_cpu_sampler_run_objective(net16.handle, arr, 1, ptr(pcn), None, ptr(noise), 2, None, None, None, 0, 2, p, q,
                                                 ptr(out), 2, 32) == -1


# ------------------------------------------------------------------------------------------------------------------
# 3. the reference's chains
# ------------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_helper_expects(golden):
    g = golden(FIXTURE)
    assert sorted(g["chains"].tolist()) == sorted(CHAINS)
    assert g["anc_normals"].shape == (40, 2, 1, 32, 32) and g["ddim5_normals"].shape == (5, 2, 1, 32, 32)
    for name in CHAINS:
        a, b = g[name + "_out"], g[name + "_out_1thread"]
        assert float(((a > 0) & (a < 1)).mean()) >= 0.6 and float(np.abs(a - b).max()) <= FP32_TOL / 4
    kp = g["pred_noise_cosine_anc_dropout_keep_p"]
    assert kp.dtype == np.float32 and np.array_equal(kp, np.full(8, 0.3, dtype=np.float32))


@pytest.mark.parametrize("name", list(CHAINS))
def test_reference_chains_on_the_twin(golden, net16, name):
    g = golden(FIXTURE)
    d = diffusion(cpu.GaussianDiffusion, net16, name, g)
    out = run(d, name, g, T).numpy()
    e = check_chain(out, g, name)
    e1 = float(np.abs(out.astype(np.float64) - g[name + "_out_1thread"]).max())
    print(f"{name}: |twin - reference|max = {e:.3e} (8 threads), {e1:.3e} (1 thread)")
    if CHAINS[name][0] != "pred_x0":                           # and the objective matters: as pred_x0 the chain is another image
        o, s, _smp, _r, _dr = CHAINS[name]
        d.objective = "pred_x0"
        assert float(np.abs(run(d, name, g, T).numpy() - g[name + "_out"]).max()) > 100 * FP32_TOL


# ------------------------------------------------------------------------------------------------------------------
# 4. pred_x0 / sigmoid is what it was
# ------------------------------------------------------------------------------------------------------------------
def test_default_model_gives_the_bits_of_run_keep(golden, net16):
    g = golden("G9_G10_sampler")
    d = cpu.GaussianDiffusion(net16, image_size=32, timesteps=8)
    assert d._objective_c(False) == (0, None, None)
    front = d.sample(param_cond=T(g["pc"]), img_cond=T(g["cond"]), noise=T(g["chain8_noise"])).numpy()
    lib = cpu.load()
    arr, n = d._steps_c(False)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    pc, cond, nz = f32(g["pc"]), f32(g["cond"]), f32(g["chain8_noise"])
    junk = np.full(n, 123.0, dtype=np.float32)

    def call(fn, *tail):
        out = np.empty((2, 1, 32, 32), dtype=np.float32)
        cpu.check(fn(net16.handle, arr, n, ptr(pc), ptr(cond), ptr(nz), len(nz), None, None, None, 0, *tail, ptr(out), 2, 32))
        return out

    keep = call(lib.prg_cpu_sampler_run_keep)
    assert np.array_equal(front, keep)
    assert np.array_equal(call(lib.prg_cpu_sampler_run_objective, 0, None, None), keep)
    assert np.array_equal(call(lib.prg_cpu_sampler_run_objective, 0, ptr(junk), ptr(junk)), keep)      # p, q ignored
    plain = np.empty_like(keep)
    cpu.check(lib.prg_cpu_sampler_run(net16.handle, arr, n, ptr(pc), ptr(cond), ptr(nz), len(nz), None, ptr(plain), 2, 32))
    assert np.array_equal(plain, keep)
    assert float(np.abs(keep - g["chain8_out"]).max()) <= FP32_TOL
