"""What tests/test_objective_host.py and tests/test_gpu_objective.py share: the chains of the G24 fixture, the transition of
include/prg.h (prg_step, with the objective of prg_sampler_set_objective and the keep threshold of prg_sampler_set_keep) restated
in numpy float32, and the row kinds the product builds for each objective."""
import numpy as np

FP32_TOL = 1e-4                 # the bound the project applies to the G9_G10 / G18 / G23 chains on this network
OBJECTIVES = {"pred_x0": 0, "pred_noise": 1, "pred_v": 2}
SCHEDULES = ("sigmoid", "cosine", "linear")
BUFFERS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
           "posterior_log_variance_clipped")
P = 0.3

FULL = (("pred_noise", "cosine"), ("pred_v", "linear"), ("pred_x0", "cosine"))
ONE = {("pred_noise", "linear"): ("ddim5", False), ("pred_noise", "sigmoid"): ("anc", True), ("pred_v", "cosine"): ("ddim5", True),
       ("pred_v", "sigmoid"): ("anc", False), ("pred_x0", "linear"): ("anc", False)}


def anc_T(schedule):
    """The short ancestral chain: the linear schedule needs 21 timesteps for its betas to stay below 1."""
    return 40 if schedule == "linear" else 8


def _chains():
    """name -> (objective, schedule, sampler, refine, dropout): tools/make_goldens.py, g24_objectives."""
    c = {}
    for o, s in FULL:
        for smp in ("anc", "ddim5"):
            for r in (False, True):
                c[f"{o}_{s}_{smp}{'_refine' if r else ''}"] = (o, s, smp, r, 0.0)
    for (o, s), (smp, r) in ONE.items():
        c[f"{o}_{s}_{smp}{'_refine' if r else ''}"] = (o, s, smp, r, 0.0)
    c["pred_noise_cosine_anc_dropout"] = ("pred_noise", "cosine", "anc", False, P)
    return c


CHAINS = _chains()


def diffusion(cls, net, name, g):
    """The chain's GaussianDiffusion (GPU front-end or CPU twin).  DDIM tables take their coefficients from the host the fixture
    was generated on (its `<schedule>_ddim5_rows`), like every other comparison with a golden DDIM chain."""
    o, s, smp, _refine, dropout = CHAINS[name]
    kw = dict(timesteps=anc_T(s)) if smp == "anc" else dict(timesteps=1000, sampling_timesteps=5)
    d = cls(net, image_size=32, objective=o, beta_schedule=s, ddnm_sampling_dropout=dropout, **kw)
    if smp == "ddim5":
        rows = d.step_table()
        assert [r["t"] for r in rows] == g[s + "_ddim5_t"].tolist()
        for r, v in zip(rows, g[s + "_ddim5_rows"]):
            for j, k in enumerate(("c_x0", "c_x", "c_eps", "sigma", "sqrt_recip", "sqrt_recipm1")):
                r[k] = float(v[j])
        d.step_table = lambda: rows
    return d


def run(d, name, g, to, **kw):
    """The chain with the fixture's stored normals (and uniforms); `to` moves a numpy array to the front-end's device."""
    _o, _s, smp, refine, dropout = CHAINS[name]
    if dropout:
        kw["keep_draws"] = to(g[name + "_uniforms"])
    return d.sample(param_cond=to(g["pc"]), img_cond=to(g["cond"]), noise=to(g[smp + "_normals"][:d.n_draws]),
                    has_refine_step=refine, **kw)


def known_mask(cond):
    return (np.asarray(cond)[:, 1:2] + np.float32(1)) * np.float32(0.5) > np.float32(0.5)


def exact_pixels(g, name):
    """Pixels of a chain without a refine row that leave the sampler as the condition: known, and kept by the last transition."""
    known = known_mask(g["cond"])
    if CHAINS[name][4]:
        u, p = g[name + "_uniforms"][-1], g[name + "_keep_p"][-1]
        assert p >= 0
        return known & (u > np.float32(p))
    return known


def check_chain(out, g, name):
    """|out - reference|max <= FP32_TOL against the 8-thread output; known-and-kept pixels of non-refine chains exact."""
    ref = g[name + "_out"]
    e = float(np.abs(np.asarray(out, dtype=np.float64) - ref).max())
    assert np.isfinite(out).all() and e <= FP32_TOL, (name, e)
    if not CHAINS[name][3]:
        px = exact_pixels(g, name)
        assert px.any() and np.array_equal(np.asarray(out)[px], ref[px]), name
    return e


# ------------------------------------------------------------------------------------------------------------------
# include/prg.h, prg_step, in numpy float32
# ------------------------------------------------------------------------------------------------------------------
def clamp_np(v):
    return np.clip(v, np.float32(-1.0), np.float32(1.0))        # propagates NaN, like torch.clamp


def reference_step(row, x, u, cond, n, objective=0, p=0.0, q=0.0, keep_p=-1.0, ku=None):
    """One transition in float32 with one rounding per operation (separate multiplies, subtraction, additions), in the order of
    include/prg.h; terms whose coefficient is zero are not added, as the kernel skips them.  x, u, n, ku (B,HW); cond (B,2,HW)."""
    f = np.float32
    x, u, n = x.astype(f), u.astype(f), n.astype(f)
    clip = int(row["clip_pred"])
    with np.errstate(invalid="ignore", over="ignore"):
        if objective:
            a = f(p) * x
            b = f(q) * u
            x0r = a - b
        else:
            x0r = u
        x0p = clamp_np(x0r) if clip & 1 else x0r
        known = np.zeros(x.shape, dtype=bool) if cond is None else (cond[:, 1] + f(1.0)) * f(0.5) > f(0.5)
        if clip & 4:                                            # the refine row ignores the keep table
            return np.where(known, clamp_np(x0r), x)
        repl = known & (ku > f(keep_p)) if (cond is not None and f(keep_p) >= 0) else known
        x0 = np.where(repl, cond[:, 0], x0p) if cond is not None else x0p
        if clip & 2:
            x0 = clamp_np(x0)
        v = f(row["c_x0"]) * x0
        if f(row["c_x"]) != 0:
            v = v + f(row["c_x"]) * x
        if f(row["c_eps"]) != 0:
            eps = u if objective == 1 else (f(row["sqrt_recip"]) * x - x0p) / f(row["sqrt_recipm1"])
            v = v + f(row["c_eps"]) * eps
        if f(row["sigma"]) != 0:
            v = v + f(row["sigma"]) * n
    assert v.dtype == np.float32
    return v


class FakeNet:
    """What GaussianDiffusion reads of its network when it only builds tables."""
    random_or_learned_sinusoidal_cond = False
    channels = out_dim = 1


def rows_of(d, refine):
    """The rows of d._steps_c(refine) as dicts, each with the (p, q) pair of d.objective_table(refine) ((0, 0) for pred_x0)."""
    arr, n = d._steps_c(refine)
    tab = d.objective_table(refine) or [(0.0, 0.0)] * n
    assert len(tab) == n
    return [dict({f: getattr(arr[i], f) for f, _ in type(arr[i])._fields_}, p=tab[i][0], q=tab[i][1]) for i in range(n)]


def row_kinds(cls, objective, schedule="cosine"):
    """kind -> row (with its p, q) from the tables the product builds for this objective: one ancestral row with noise, the
    ancestral row at t = 0, a DDIM row with eps and noise, the last DDIM row, and the refine row."""
    anc = rows_of(cls(FakeNet(), image_size=32, timesteps=1000, objective=objective, beta_schedule=schedule), False)
    ddim = rows_of(cls(FakeNet(), image_size=32, timesteps=1000, sampling_timesteps=5, objective=objective,
                       beta_schedule=schedule), True)
    kinds = {"ancestral": anc[500], "ancestral_t0": anc[999], "ddim": ddim[2], "ddim_last": ddim[4], "refine": ddim[5]}
    assert kinds["ancestral"]["sigma"] != 0 and kinds["ancestral"]["clip_pred"] == 2 and kinds["ancestral_t0"]["sigma"] == 0
    assert kinds["ddim"]["c_eps"] != 0 and kinds["ddim"]["sigma"] != 0 and kinds["ddim"]["clip_pred"] == 1
    assert (kinds["ddim_last"]["c_x0"], kinds["ddim_last"]["c_eps"], kinds["ddim_last"]["sigma"]) == (1.0, 0.0, 0.0)
    assert kinds["refine"]["clip_pred"] == 4 and kinds["refine"]["t"] == 0
    return kinds
