"""objective = pred_noise / pred_v on the device: the OBJ instantiations of sampler_step_kernel (csrc/sampler.hip), the objective
table of the sampler handle, and GaussianDiffusion.sample on top of them.  Run with `-m gpu`.

What is compared with what:
  * the step kernel alone (prg_debug_sampler_step_objective) against the numpy float32 restatement of include/prg.h in
    tests/_objectives.py, fed the device's own Philox normals: bit for bit, NaN and +-Inf in the network output included.
  * objective 0 through the new hook against prg_debug_sampler_step_keep: bit for bit.
  * every reference chain of G24_objectives in fp32 and f16x3: FP32_TOL = 1e-4, the bound of the G9_G10 / G18 / G23 chains on this
    network; pixels that leave the sampler as the condition bit for bit.  bf16: finite, those pixels bit for bit, nothing else (the
    fixture cannot bound its drift).
  * graph replay against eager launches, a handle whose objective is changed between runs against fresh handles, the seeded path
    against the stored path fed the Philox oracle's draws, and the device against the C++ twin.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _ddnm_dropout import oracle_normals
from _objectives import CHAINS, FP32_TOL, OBJECTIVES, check_chain, diffusion, exact_pixels, reference_step, row_kinds, run
from pointreggpt_amd import weights as W
from test_gpu_sampler_step import GUARD, SEEDS, hip, seeds_for  # noqa: F401

pytestmark = pytest.mark.gpu

FIXTURE = "G24_objectives"
SHAPES = [(1, 4), (3, 144), (300, 2048)]        # one quad | partial workgroup | B > 256: one workgroup per image, two strides
KINDS = ["ancestral", "ancestral_t0", "ddim", "ddim_last", "refine"]
READOUT = dict(t=0, clip_pred=0, c_x0=0.0, c_x=0.0, c_eps=0.0, sigma=1.0, sqrt_recip=1.0, sqrt_recipm1=1.0)   # x' = 0 * x0 + 1 * n


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def step_c(hip, row):
    return hip._lib.StepC(int(row["t"]), int(row["clip_pred"]), row["c_x0"], row["c_x"], row["c_eps"], row["sigma"], row["sqrt_recip"],
                          row["sqrt_recipm1"])


def run_step(hip, row, x, u, cond, seeds, objective=0, p=0.0, q=0.0, keep_p=-1.0, keep_u=None, via="objective"):
    """One launch of sampler_step_kernel on host arrays; x sits between two guard rows that must come back untouched."""
    B, HW = x.shape
    buf = torch.full((B + 2, HW), GUARD, dtype=torch.float32, device="cuda")
    buf[1:B + 1] = D(np.asarray(x, dtype=np.float32))
    xin = buf[1:B + 1]
    ud = D(np.asarray(u, dtype=np.float32))
    cd = None if cond is None else D(np.asarray(cond, dtype=np.float32))
    sd = D(np.array(seeds, dtype=np.uint64).view(np.int64))
    kd = None if keep_u is None else D(np.asarray(keep_u, dtype=np.float32).reshape(1, B, HW))
    rc = step_c(hip, row)
    L = hip._lib
    f = lambda v: float(np.float32(v))
    if via == "keep":
        L.check(hip.lib.prg_debug_sampler_step_keep(L.ptr(xin), L.ptr(ud), L.ptr(cd), L.ptr(sd), C.byref(rc), f(keep_p), L.ptr(kd), B, HW,
                                                    1, None, None), "prg_debug_sampler_step_keep")
    else:
        L.check(hip.lib.prg_debug_sampler_step_objective(L.ptr(xin), L.ptr(ud), L.ptr(cd), L.ptr(sd), C.byref(rc), int(objective), f(p),
                                                         f(q), f(keep_p), L.ptr(kd), B, HW, 1, None, None),
                "prg_debug_sampler_step_objective")
    out = buf.cpu().numpy()
    assert np.all(out[0] == GUARD) and np.all(out[-1] == GUARD), "sampler_step_kernel wrote outside x"
    return out[1:B + 1].copy()


@pytest.fixture(scope="module")
def inputs(hip):
    """(B, HW) -> x, u, cond, uniforms, draw 1 of the device, poison mask.  u in +-3 (so that x0r = p * x - q * u leaves [-1, 1] on
    about half the pixels), NaN, +Inf, -Inf planted on the first known and the first in-painted pixels of every image; condition
    depth in +-1.5; mask channel over {-1, 1, 0, 1e-7, -1e-7}; uniforms on the 2^-24 grid."""
    cache = {}

    def get(B, HW):
        if (B, HW) not in cache:
            g = np.random.default_rng(2400 + B)
            x = (g.standard_normal((B, HW)) * 1.5).astype(np.float32)
            u = g.uniform(-3, 3, (B, HW)).astype(np.float32)
            cond = np.empty((B, 2, HW), dtype=np.float32)
            cond[:, 0] = g.uniform(-1.5, 1.5, (B, HW))
            cond[:, 1] = np.array([-1.0, 1.0, 0.0, 1e-7, -1e-7], dtype=np.float32)[g.integers(0, 5, (B, HW))]
            cond[:, 1, :4] = np.array([1.0, -1.0, 1e-7, 0.0], dtype=np.float32)       # every image has both kinds, also at HW = 4
            known = (cond[:, 1] + np.float32(1)) * np.float32(0.5) > np.float32(0.5)
            poison = np.zeros((B, HW), dtype=bool)
            bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
            for b in range(B):
                for idx in (np.flatnonzero(known[b])[:3], np.flatnonzero(~known[b])[:3]):
                    assert len(idx) >= 2
                    u[b, idx] = bad[:len(idx)]
                    poison[b, idx] = True
            ku = (g.integers(0, 2 ** 24, (B, HW)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
            z = np.zeros((B, HW), dtype=np.float32)
            n1 = run_step(hip, READOUT, z, z, None, seeds_for(B))
            assert np.isfinite(n1).all() and float(n1.std()) > 0.5
            cache[(B, HW)] = (x, u, cond, ku, n1, poison)
        return cache[(B, HW)]

    return get


# ------------------------------------------------------------------------------------------------------------------
# 1. the step kernel alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("objective", ["pred_noise", "pred_v"])
def test_every_row_kind_with_an_objective(hip, inputs, objective, kind):
    code = OBJECTIVES[objective]
    row = row_kinds(hip.GaussianDiffusion, objective)[kind]
    p, q = row["p"], row["q"]
    for B, HW in SHAPES:
        x, u, cond, ku, n1, poison = inputs(B, HW)
        seeds = seeds_for(B)
        if HW >= 144:
            x0r = np.float32(p) * x[~poison] - np.float32(q) * u[~poison]
            assert 0.2 < float((np.abs(x0r) > 1).mean()) < 0.8, (objective, kind)
        got = {}
        for with_cond in (True, False):
            c = cond if with_cond else None
            for keep_p in (-1.0, 0.3):
                out = run_step(hip, row, x, u, c, seeds, code, p, q, keep_p, ku if keep_p >= 0 else None)
                ref = reference_step(row, x, u, c, n1, code, p, q, keep_p, ku)
                assert np.array_equal(out, ref, equal_nan=True), (objective, kind, B, HW, with_cond, keep_p,
                                                                  int(((out != ref) & ~(np.isnan(out) & np.isnan(ref))).sum()))
                got[(with_cond, keep_p)] = out
        # NaN stays NaN wherever the pixel takes the network output: in-painted pixels (known ones on the refine row)
        known = (cond[:, 1] + np.float32(1)) * np.float32(0.5) > np.float32(0.5)
        nan_u = np.isnan(u)
        takes = known if kind == "refine" else ~known
        assert np.isnan(got[(True, -1.0)][nan_u & takes]).all() and (nan_u & takes).any()
        assert np.isfinite(got[(True, -1.0)][~poison]).all()
        assert np.array_equal(got[(False, -1.0)], got[(False, 0.3)], equal_nan=True)          # no condition: no keep mask
        if HW >= 144:                                                                           # (two known pixels may both be kept)
            assert np.array_equal(got[(True, -1.0)], got[(True, 0.3)], equal_nan=True) == (kind == "refine")
        plain = run_step(hip, row, x, u, cond, seeds, 0)
        assert not np.array_equal(plain, got[(True, -1.0)], equal_nan=True)                   # the objective does something


@pytest.mark.parametrize("kind", KINDS)
def test_objective_0_is_the_keep_hook(hip, inputs, kind):
    row = row_kinds(hip.GaussianDiffusion, "pred_x0")[kind]
    for B, HW in SHAPES:
        x, u, cond, ku, n1, _poison = inputs(B, HW)
        for c in (cond, None):
            for keep_p in (-1.0, 0.3):
                kw = dict(keep_p=keep_p, keep_u=ku if keep_p >= 0 else None)
                old = run_step(hip, row, x, u, c, seeds_for(B), via="keep", **kw)
                new = run_step(hip, row, x, u, c, seeds_for(B), 0, 123.0, -7.0, **kw)          # p, q ignored
                assert np.array_equal(old, new, equal_nan=True), (kind, B, HW, c is None, keep_p)
                assert np.array_equal(new, reference_step(row, x, u, c, n1, 0, 0.0, 0.0, keep_p, ku), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------
# 2. the reference's chains
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(hip, golden):
    made = {}

    def get(dtype):
        if dtype not in made:
            net = hip.Unet(16, dtype=dtype).load_state_dict(W.synth_state_dict(W.unet_config(16), 9))
            made[dtype] = net.set_time_freqs(golden("G0_host_tables")["freqs_dim16"])
        return made[dtype]

    yield get
    for net in made.values():
        net.close()


@pytest.mark.parametrize("dtype", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_reference_chains(hip, golden, nets, name, dtype):
    g = golden(FIXTURE)
    d = diffusion(hip.GaussianDiffusion, nets(dtype), name, g)
    out = run(d, name, g, D).cpu().numpy()
    again = run(d, name, g, D).cpu().numpy()
    d.close()
    e = float(np.abs(out.astype(np.float64) - g[name + "_out"]).max())
    print(f"{name} {dtype}: |hip - reference|max = {e:.3e}")
    check_chain(out, g, name)
    assert np.array_equal(out, again)


@pytest.mark.parametrize("name", list(CHAINS))
def test_reference_chains_bf16_stay_finite_and_keep_the_condition(hip, golden, nets, name):
    g = golden(FIXTURE)
    d = diffusion(hip.GaussianDiffusion, nets("bf16"), name, g)
    out = run(d, name, g, D).cpu().numpy()
    d.close()
    assert np.isfinite(out).all()
    if not CHAINS[name][3]:
        px = exact_pixels(g, name)
        assert px.any() and np.array_equal(out[px], g[name + "_out"][px])


@pytest.mark.parametrize("name", ["pred_noise_cosine_anc", "pred_v_linear_ddim5_refine"])
def test_graph_replay_equals_eager_launches(hip, golden, nets, name):
    g = golden(FIXTURE)
    d = diffusion(hip.GaussianDiffusion, nets("fp32"), name, g)
    eager = run(d, name, g, D, use_graph=False).cpu().numpy()
    graph = run(d, name, g, D, use_graph=True).cpu().numpy()
    replay = run(d, name, g, D, use_graph=True).cpu().numpy()
    d.close()
    check_chain(graph, g, name)
    assert np.array_equal(eager, graph) and np.array_equal(graph, replay)


# ------------------------------------------------------------------------------------------------------------------
# 3. the handle
# ------------------------------------------------------------------------------------------------------------------
def test_one_handle_follows_its_objective(hip, golden, nets):
    """set, run, set something else, run: every run of the one handle (captured graph and all) is a fresh handle's, bit for bit."""
    g = golden(FIXTURE)
    net = nets("fp32")
    kw = dict(param_cond=D(g["pc"]), img_cond=D(g["cond"]), noise=D(g["anc_normals"][:8]), use_graph=True)
    fresh, tabs = {}, {}
    for o in OBJECTIVES:
        d = hip.GaussianDiffusion(net, image_size=32, timesteps=8, objective=o, beta_schedule="cosine")
        fresh[o] = d.sample(**kw).cpu().numpy()
        tabs[o] = d._objective_c(False)
        d.close()
    assert not np.array_equal(fresh["pred_noise"], fresh["pred_v"]) and not np.array_equal(fresh["pred_x0"], fresh["pred_v"])
    d = hip.GaussianDiffusion(net, image_size=32, timesteps=8, objective="pred_noise", beta_schedule="cosine")
    assert np.array_equal(d.sample(**kw).cpu().numpy(), fresh["pred_noise"])
    h = d._sampler(2, False, "sample")
    L, lib = hip._lib, hip.lib
    for o in ("pred_v", "pred_x0", "pred_noise", "pred_noise", "pred_x0", "pred_v"):
        code, p, q = tabs[o]
        L.check(lib.prg_sampler_set_objective(h, code, p, q, 8 if code else 0), "prg_sampler_set_objective")
        assert np.array_equal(d.sample(**kw).cpu().numpy(), fresh[o]), o
        assert np.array_equal(d.sample(**kw).cpu().numpy(), fresh[o]), o                # replay
    # refusals leave the handle as it was (pred_v)
    code, p, q = tabs["pred_noise"]
    for args in ((code, p, q, 7), (code, p, q, 9), (code, None, q, 8), (code, p, None, 8), (3, p, q, 8), (-1, p, q, 8)):
        assert lib.prg_sampler_set_objective(h, *args) == -1 and b"prg_sampler_set_objective" in lib.prg_last_error()
    assert np.array_equal(d.sample(**kw).cpu().numpy(), fresh["pred_v"])
    # the same objective with another table: the captured graph reads the new one
    code, p, q = tabs["pred_v"]
    swapped = (C.c_float * 8)(*list(q)), (C.c_float * 8)(*list(p))
    L.check(lib.prg_sampler_set_objective(h, code, swapped[0], swapped[1], 8))
    other = d.sample(**kw).cpu().numpy()
    assert not np.array_equal(other, fresh["pred_v"])
    L.check(lib.prg_sampler_set_objective(h, code, p, q, 8))
    assert np.array_equal(d.sample(**kw).cpu().numpy(), fresh["pred_v"])
    d.close()


def test_seeded_run_is_the_stored_run_fed_the_oracles_draws(hip, golden, nets):
    g = golden(FIXTURE)
    seeds = [SEEDS[3], SEEDS[2]]
    d = hip.GaussianDiffusion(nets("fp32"), image_size=32, timesteps=8, objective="pred_noise", beta_schedule="cosine")
    kw = dict(param_cond=D(g["pc"]), img_cond=D(g["cond"]))
    for graph in (False, True):
        seeded = d.sample(seeds=seeds, use_graph=graph, **kw).cpu().numpy()
        stored = d.sample(noise=oracle_normals(seeds, 0, d.n_draws, 32).cuda(), use_graph=graph, **kw).cpu().numpy()
        shifted = d.sample(noise=oracle_normals(seeds, 1, d.n_draws, 32).cuda(), use_graph=graph, **kw).cpu().numpy()
        e = float(np.abs(seeded - stored).max())
        print(f"pred_noise / cosine T8 graph={graph}: |seeded - stored|max = {e:.3e}")
        assert np.isfinite(seeded).all() and e <= FP32_TOL
        assert float(np.abs(seeded - shifted).max()) > 1000 * FP32_TOL
    d.close()


@pytest.mark.parametrize("name", ["pred_noise_cosine_ddim5", "pred_v_linear_anc", "pred_x0_cosine_anc_refine"])
def test_device_against_the_cpu_twin(hip, golden, nets, name):
    from pointreggpt_amd import cpu
    g = golden(FIXTURE)
    twin_net = cpu.Unet(16).load_state_dict(W.synth_state_dict(W.unet_config(16), 9)).set_time_freqs(golden("G0_host_tables")["freqs_dim16"])
    dc = diffusion(cpu.GaussianDiffusion, twin_net, name, g)
    twin = run(dc, name, g, torch.tensor).numpy()
    twin_net.close()
    d = diffusion(hip.GaussianDiffusion, nets("fp32"), name, g)
    out = run(d, name, g, D).cpu().numpy()
    d.close()
    e = float(np.abs(out.astype(np.float64) - twin).max())
    print(f"{name}: |hip - twin|max = {e:.3e}")
    assert e <= FP32_TOL
