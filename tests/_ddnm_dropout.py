"""What tests/test_ddnm_dropout_host.py and tests/test_gpu_ddnm_dropout.py share: the six chains of the G23 fixture, the keep-mask
uniforms restated from include/prg.h on top of the raw Philox oracle (oracle/philox.py), and the stored draws of a seeded run."""
import numpy as np
import torch

from oracle import philox as PH

FP32_TOL = 1e-4                 # the bound tests/test_cpu_twins.py and tests/test_gpu_parity.py apply to the G9_G10 / G18 chains
DOMAIN_KEEP = 0x6B656570        # third counter word of the keep-mask draws; the normals use PH.DOMAIN
P = 0.3

# name -> constructor keywords, refine, method (tools/make_goldens.py, g23_ddnm_dropout)
CHAINS = {
    "T8_linear": (dict(timesteps=8, ddnm_dropout_schedule="linear"), False, "sample"),
    "T8_none_refine": (dict(timesteps=8, ddnm_dropout_schedule="none"), True, "sample"),
    "ddim5_none": (dict(timesteps=1000, sampling_timesteps=5, ddnm_dropout_schedule="none"), False, "sample"),
    "ddim5_linear_refine": (dict(timesteps=1000, sampling_timesteps=5, ddnm_dropout_schedule="linear"), True, "sample"),
    "denoise_T8": (dict(timesteps=8, is_ddnm_sampling=False), False, "denoise"),
    "denoise_ddim5_refine": (dict(timesteps=1000, sampling_timesteps=5, is_ddnm_sampling=False), True, "denoise"),
}
# uniform_ draws the reference made per chain (the issue's count, from the semantics; the fixture must show the same)
N_DRAWS = {"T8_linear": 7, "T8_none_refine": 8, "ddim5_none": 5, "ddim5_linear_refine": 4, "denoise_T8": 8, "denoise_ddim5_refine": 5}


def diffusion(cls, net, name, golden):
    """The chain's GaussianDiffusion (GPU front-end or CPU twin).  DDIM tables take their coefficients from the host the
    fixtures were generated on (G0_host_tables), like every other comparison with a golden DDIM chain."""
    kw, _refine, _method = CHAINS[name]
    d = cls(net, image_size=32, ddnm_sampling_dropout=P, **kw)
    if "sampling_timesteps" in kw:
        g0 = golden("G0_host_tables")
        rows = d.step_table()
        assert [r["t"] for r in rows] == g0["ddim5_t"].tolist()
        for r, v in zip(rows, g0["ddim5_rows"]):
            for j, k in enumerate(("c_x0", "c_x", "c_eps", "sigma", "sqrt_recip", "sqrt_recipm1")):
                r[k] = float(v[j])
        d.step_table = lambda: rows
    return d


def normals_of(g, name):
    return g["ddim5_normals" if "ddim5" in name else "T8_normals"]


def run(d, name, g, to, uniforms=None, **kw):
    """The chain with the fixture's stored normals and uniforms; `to` moves a numpy array to the front-end's device."""
    _kw, refine, method = CHAINS[name]
    u = g[name + "_uniforms"] if uniforms is None else uniforms
    return getattr(d, method)(param_cond=to(g["pc"]), img_cond=to(g["cond"]), noise=to(normals_of(g, name)), keep_draws=to(u),
                              has_refine_step=refine, **kw)


def known_mask(cond):
    return (np.asarray(cond)[:, 1:2] + np.float32(1)) * np.float32(0.5) > np.float32(0.5)


def last_kept(g, name):
    """Pixels known AND kept in the last transition of a chain without a refine row: they leave the sampler as the condition."""
    u, p = g[name + "_uniforms"][-1], g[name + "_keep_p"][-1]
    assert p >= 0
    return known_mask(g["cond"]) & (u > np.float32(p))


def keep_masks(keep_p, draws, cond):
    """Row k -> the pixels transition k replaces when fed `draws` (rows,B,1,S,S): known & (u > keep_p[k]) in float32; all known
    pixels on a row without a threshold."""
    known = known_mask(cond)
    u = np.asarray(draws, dtype=np.float32)
    return [known & (u[k] > np.float32(p)) if p >= 0 else known for k, p in enumerate(np.asarray(keep_p, dtype=np.float32))]


def check_denoise_masks(d, refine, draws_a, draws_b, cond, out_a, out_b):
    """What a change of uniforms can do to denoise() on a model without is_ddnm_sampling: denoise_dropouts = linspace(1, 0, T) ** 100,
    indexed by t, is 1 at t = 0 (the ancestral sampler's last transition; u > 1 never: nothing is kept) and at most 2^-22 elsewhere (everything is kept
    but the few u at or below it; u == 0 alone where it underflows to 0).  So two sets of uniforms give the same masks unless one
    of them holds such a u on a known pixel, and equal masks with equal normals are equal chains, bit for bit."""
    kp = np.array(d.keep_table("denoise", refine), dtype=np.float32)
    n = len(kp) - int(refine)
    ts = [r["t"] for r in d.step_table()]
    assert all(p == 1.0 if t == 0 else 0 <= p <= 2.0 ** -22 for t, p in zip(ts, kp[:n])) and (kp[n:] == -1.0).all()
    known = known_mask(cond)
    ma, mb = keep_masks(kp[:n], draws_a, cond), keep_masks(kp[:n], draws_b, cond)
    for k in range(n):
        if kp[k] == 1.0:
            assert not ma[k].any() and not mb[k].any()
            continue
        for m, u in ((ma[k], np.asarray(draws_a)[k]), (mb[k], np.asarray(draws_b)[k])):
            assert np.array_equal(m, known & (u != 0)) if kp[k] == 0 else (m | ~known).mean() > 0.999
    same = all(np.array_equal(a, b) for a, b in zip(ma, mb))
    assert np.array_equal(out_a, out_b) == same, same


def keep_uniforms(key: int, draw: int, n_pixels: int, domain: int = DOMAIN_KEEP) -> np.ndarray:
    """include/prg.h, prg_sampler_set_keep_draws: counter {quad, draw, domain, 0} under the scene key; word i >> 8, times 2^-24,
    is pixel 4 * quad + i's uniform.  Exact in float32 (24-bit integers), so the device has to match bit for bit."""
    assert n_pixels % 4 == 0
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    quad = np.arange(n_pixels // 4, dtype=np.uint64)
    zero = np.zeros_like(quad)
    words = PH.philox4x32_10((quad, zero + np.uint64(draw), zero + np.uint64(domain), zero), (key & 0xFFFFFFFF, key >> 32))
    k = np.stack([w >> np.uint64(8) for w in words], axis=1).reshape(-1)
    u = k.astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, k.astype(np.float64))
    return u


def oracle_normals(seeds, first, count, S):
    """(count, B, 1, S, S): slab k = float32(oracle normal draw first + k) of every seed."""
    return torch.from_numpy(np.stack([np.stack([PH.normals(s, first + k, S * S)[0].astype(np.float32).reshape(1, S, S) for s in seeds])
                                      for k in range(count)]))


def oracle_keep_draws(seeds, first, count, S):
    """(count, B, 1, S, S): slab k = keep draw first + k + 1 of every seed: what transition k consumes when first = 0."""
    return torch.from_numpy(np.stack([np.stack([keep_uniforms(s, first + k + 1, S * S).reshape(1, S, S) for s in seeds])
                                      for k in range(count)]))
