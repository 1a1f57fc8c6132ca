"""Stochastic DDNM (ddnm_sampling_dropout / ddnm_dropout_schedule, sd:1075-1094, 1210-1227) and denoise() (sd:1411-1427) without a
GPU: the host tables against the thresholds the reference itself compared its draws with, and the C++ twin
(prg_cpu_sampler_run_keep) against the six reference chains of G23_ddnm_dropout, stored and seeded.

Tolerances: thresholds exact (float32); chains <= FP32_TOL = 1e-4, the bound tests/test_cpu_twins.py applies to the G9_G10 / G18
chains on this network; pixels that leave the sampler as the condition, and repeated runs, bit for bit."""
import numpy as np
import pytest
import torch

from _ddnm_dropout import check_denoise_masks, CHAINS, FP32_TOL, N_DRAWS, P, diffusion, keep_uniforms, known_mask, last_kept, oracle_keep_draws, \
    oracle_normals, run
from pointreggpt_amd import cpu
from pointreggpt_amd import weights as W
from pointreggpt_amd.diffusion import GaussianDiffusion

T = torch.tensor


class _FakeNet:
    channels = out_dim = 1
    random_or_learned_sinusoidal_cond = False


def maxerr(a, b):
    return float(np.nanmax(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


# ------------------------------------------------------------------------------------------------------------------
# 1. host tables
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CHAINS))
def test_keep_table_is_the_references(golden, name):
    g = golden("G23_ddnm_dropout")
    kw, refine, method = CHAINS[name]
    d = GaussianDiffusion(_FakeNet(), image_size=32, ddnm_sampling_dropout=float(g["p"]), **kw)
    keep = np.array(d.keep_table(method, refine), dtype=np.float32)
    ref = g[name + "_keep_p"]
    assert ref.dtype == np.float32 and len(keep) == d._steps_c(refine)[1] == len(ref)
    assert np.array_equal(keep, ref), (name, keep, ref)
    # the drawing rows are the ones for which the reference drew, and as many as the semantics predict
    drew = ~np.isnan(g[name + "_uniforms"]).reshape(len(ref), -1).all(axis=1)
    assert np.array_equal(keep >= 0, drew) and int(drew.sum()) == N_DRAWS[name]
    assert not np.isnan(g[name + "_uniforms"][drew]).any()
    c = d._keep_c(method, refine)
    assert c is not None and np.array_equal(np.ctypeslib.as_array(c), ref)
    if refine:
        assert keep[-1] == -1.0
    if method == "denoise":                       # denoise_dropouts = linspace(1, 0, T) ** 100: always a draw, mostly against 0
        assert (keep[:len(keep) - int(refine)] >= 0).all() and (keep == 0).any()
        assert d.keep_table("sample", refine) == [-1.0] * len(ref)        # sample() of such a model has no DDNM at all


def test_tables_and_rejections():
    d = GaussianDiffusion(_FakeNet(), image_size=32, timesteps=8, ddnm_sampling_dropout=P, ddnm_dropout_schedule="linear")
    assert d.ddnm_dropouts.dtype == torch.float64 and d.denoise_dropouts.dtype == torch.float64
    assert torch.equal(d.ddnm_dropouts, torch.linspace(P, 0.0, 8, dtype=torch.float64))
    assert torch.equal(d.denoise_dropouts, torch.linspace(1.0, 0.0, 8, dtype=torch.float64) ** 100)
    assert d.keep_table("sample")[0] == -1.0 and d.keep_table("sample")[-1] == float(np.float32(P))     # t = T - 1 has p = 0
    d = GaussianDiffusion(_FakeNet(), image_size=32, timesteps=8, ddnm_sampling_dropout=P)
    assert torch.equal(d.ddnm_dropouts, torch.full((8,), P, dtype=torch.float64))
    assert d.keep_table("denoise", True) == d.keep_table("sample", True) == [float(np.float32(P))] * 8 + [-1.0]
    for bad in (dict(ddnm_dropout_schedule="cosine"), dict(ddnm_sampling_dropout=-0.1), dict(ddnm_sampling_dropout=1.5),
                dict(objective="pred_v"), dict(beta_schedule="linear"), dict(objective="pred_noise")):
        with pytest.raises(ValueError):
            GaussianDiffusion(_FakeNet(), image_size=32, **bad)
    with pytest.raises(ValueError):
        d.keep_table("interpolate")
    for p in (0.0, 1.0):
        GaussianDiffusion(_FakeNet(), image_size=32, ddnm_sampling_dropout=p, ddnm_dropout_schedule="linear")


@pytest.mark.parametrize("kw", [dict(timesteps=8), dict(timesteps=1000, sampling_timesteps=5)])
def test_zero_dropout_is_the_plain_sampler(kw):
    """Dropout 0: the same transition table, byte for byte, as a model built without the keywords (and as one with dropout: the
    table does not depend on it), and no keep table at all, for sample() and for denoise()."""
    plain = GaussianDiffusion(_FakeNet(), image_size=32, **kw)
    zero = GaussianDiffusion(_FakeNet(), image_size=32, ddnm_sampling_dropout=0.0, ddnm_dropout_schedule="linear", **kw)
    some = GaussianDiffusion(_FakeNet(), image_size=32, ddnm_sampling_dropout=P, **kw)
    for refine in (False, True):
        a, n = plain._steps_c(refine)
        for d in (zero, some):
            b, m = d._steps_c(refine)
            assert n == m and bytes(a) == bytes(b)
        for d in (plain, zero):
            for mode in ("sample", "denoise"):
                assert d.keep_table(mode, refine) == [-1.0] * n and d._keep_c(mode, refine) is None
        assert some._keep_c("sample", refine) is not None


# ------------------------------------------------------------------------------------------------------------------
# 2. the C++ twin against the reference's chains
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(golden):
    n = cpu.Unet(16).load_state_dict(W.synth_state_dict(W.unet_config(16), 9))
    yield n.set_time_freqs(golden("G0_host_tables")["freqs_dim16"])
    n.close()


def test_fixture_is_what_the_issue_asks_for(golden):
    g = golden("G23_ddnm_dropout")
    g9 = golden("G9_G10_sampler")
    assert np.array_equal(g["pc"], g9["pc"]) and np.array_equal(g["cond"], g9["cond"]) and float(g["p"]) == P
    for name in CHAINS:
        out = g[name + "_out"]
        inside = float(((out > 0) & (out < 1)).mean())
        assert inside >= 0.6, (name, inside)
        u = g[name + "_uniforms"]
        drew = g[name + "_keep_p"] >= 0
        assert u.dtype == np.float32 and (u[drew] >= 0).all() and (u[drew] < 1).all()
        assert np.array_equal(u[drew] * np.float32(2 ** 24), np.round(u[drew] * np.float32(2 ** 24)))      # the 2^-24 grid


@pytest.mark.parametrize("name", list(CHAINS))
def test_cpu_twin_reproduces_the_reference_chain(golden, net, name):
    g = golden("G23_ddnm_dropout")
    _kw, refine, method = CHAINS[name]
    d = diffusion(cpu.GaussianDiffusion, net, name, golden)
    out = run(d, name, g, T).numpy()
    e = maxerr(out, g[name + "_out"])
    print(f"{name}: |cpu twin - reference|max = {e:.3e}")
    assert e <= FP32_TOL, (name, e)
    if method == "sample" and not refine:
        kept = last_kept(g, name)
        known = known_mask(g["cond"])
        assert kept.any() and (known & ~kept).any() and np.array_equal(out[kept], g[name + "_out"][kept])
    # the NaN slabs (rows for which the reference drew nothing) are never read
    zeros = np.nan_to_num(g[name + "_uniforms"], nan=0.0)
    assert np.isnan(g[name + "_uniforms"]).any() == (N_DRAWS[name] < len(g[name + "_keep_p"]))
    assert np.array_equal(run(d, name, g, T, uniforms=zeros).numpy(), out)
    # and the table is not ignored: uniforms of 0 keep nothing (u > p is false for every p >= 0), which is another chain
    none_kept = np.where(np.isnan(g[name + "_uniforms"]), np.float32(np.nan), np.float32(0)).astype(np.float32)
    assert maxerr(run(d, name, g, T, uniforms=none_kept).numpy(), out) > 100 * FP32_TOL
    # too few keep slabs for the table
    with pytest.raises((AssertionError, cpu._hip.PrgError)):
        run(d, name, g, T, uniforms=g[name + "_uniforms"][:1])


# ------------------------------------------------------------------------------------------------------------------
# 3. the C++ twin, seeded
# ------------------------------------------------------------------------------------------------------------------
def test_keep_uniform_oracle_is_a_stream_of_its_own():
    u = keep_uniforms(7, 1, 4096)
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1 and abs(float(u.mean()) - 0.5) < 6 * np.sqrt(1 / 12 / 4096)
    assert not np.array_equal(u, keep_uniforms(7, 2, 4096)) and not np.array_equal(u, keep_uniforms(8, 1, 4096))
    from oracle import philox as PH
    assert not np.array_equal(u, keep_uniforms(7, 1, 4096, domain=PH.DOMAIN))


@pytest.mark.parametrize("name", ["T8_linear", "ddim5_none", "denoise_T8", "denoise_ddim5_refine"])
def test_cpu_twin_seeded_equals_stored_oracle_draws(golden, net, name):
    """sample(seeds=) / denoise(seeds=): transition k takes keep draw k + 1 and normal draw k + 1 of its scene's key, the start
    image normal draw 0.  The uniforms are exact, the twin's normals are libm's (within float32 roundoff of the oracle's)."""
    g = golden("G23_ddnm_dropout")
    _kw, refine, method = CHAINS[name]
    seeds = [5, 2 ** 40 + 3]
    d = diffusion(cpu.GaussianDiffusion, net, name, golden)
    n_rows = len(g[name + "_keep_p"])
    call = getattr(d, method)
    kw = dict(param_cond=T(g["pc"]), img_cond=T(g["cond"]), has_refine_step=refine)
    seeded = call(seeds=seeds, **kw).numpy()
    stored = call(noise=oracle_normals(seeds, 0, d.n_draws, 32), keep_draws=oracle_keep_draws(seeds, 0, n_rows, 32), **kw).numpy()
    half = call(noise=oracle_normals(seeds, 0, d.n_draws, 32), seeds=seeds, **kw).numpy()        # stored normals, Philox keep mask
    shifted = call(noise=oracle_normals(seeds, 0, d.n_draws, 32), keep_draws=oracle_keep_draws(seeds, 1, n_rows, 32), **kw).numpy()
    e = maxerr(seeded, stored)
    print(f"{name}: |seeded - stored oracle draws|max = {e:.3e}")
    assert e <= FP32_TOL and np.array_equal(half, stored)
    assert np.array_equal(call(seeds=seeds, **kw).numpy(), seeded)
    if method == "sample":      # (denoise: check_denoise_masks below)
        known = known_mask(g["cond"])
        assert float((shifted != stored)[known].mean()) > 0.01
    else:
        check_denoise_masks(d, refine, oracle_keep_draws(seeds, 0, n_rows, 32).numpy(), oracle_keep_draws(seeds, 1, n_rows, 32).numpy(),
                            g["cond"], stored, shifted)
