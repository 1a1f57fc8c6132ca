"""Host-side mirror of ``GaussianDiffusion`` (sd:1015-1409) for sampling, backed by the HIP sampler.

The float64 schedule and the per-transition coefficients are computed here with torch exactly as the
reference computes them (tiny, one-off); the library receives them as a ``prg_step`` table and runs the
whole chain on the GPU: U-Net + fused update per transition, captured once as a hipGraph and replayed.
sd = /root/reference/denoising_diffusion_pytorch/successive_ddnm_diffusion.py
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .unet import Unet


def sigmoid_beta_schedule(timesteps: int, start=-3, end=3, tau=1) -> torch.Tensor:
    """Sigmoid alpha-bar schedule, float64, betas clipped to [0, 0.999] (sd:997-1012)."""
    t = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64) / timesteps
    v_start = torch.tensor(start / tau).sigmoid()
    v_end = torch.tensor(end / tau).sigmoid()
    ac = (-((t * (end - start) + start) / tau).sigmoid() + v_end) / (v_end - v_start)
    ac = ac / ac[0]
    return torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999)


def linear_beta_schedule(timesteps: int) -> torch.Tensor:
    """Linear betas scaled by 1000 / timesteps, float64, NOT clipped (sd:976-980): below 21 timesteps the last one exceeds 1."""
    scale = 1000 / timesteps
    return torch.linspace(scale * 0.0001, scale * 0.02, timesteps, dtype=torch.float64)


def cosine_beta_schedule(timesteps: int, s=0.008) -> torch.Tensor:
    """Cosine alpha-bar schedule, float64, betas clipped to [0, 0.999] (sd:983-994)."""
    x = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64)
    ac = torch.cos(((x / timesteps) + s) / (1 + s) * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    return torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999)


BETA_SCHEDULES = {"linear": linear_beta_schedule, "cosine": cosine_beta_schedule, "sigmoid": sigmoid_beta_schedule}
OBJECTIVES = {"pred_x0": 0, "pred_noise": 1, "pred_v": 2}     # the codes of prg_sampler_set_objective (include/prg.h)
LOSS_TYPES = {"l1": 0, "l2": 1}                               # the codes of prg_diffusion_loss


def _schedule64(timesteps: int, beta_schedule: str):
    """The float64 betas of the named schedule and their alphas_cumprod, checked (sd:1047-1057)."""
    if beta_schedule not in BETA_SCHEDULES:
        raise ValueError(f"unknown beta schedule {beta_schedule}")
    betas = BETA_SCHEDULES[beta_schedule](timesteps)
    if bool((betas >= 1).any()):
        raise ValueError(f"beta_schedule='{beta_schedule}' with timesteps={timesteps} has a beta >= 1 "
                         f"(max {float(betas.max()):.4g}): the chain would be NaN; the linear schedule needs timesteps >= 21")
    return betas, torch.cumprod(1.0 - betas, dim=0)


def make_schedule(timesteps: int, beta_schedule: str = "sigmoid") -> Dict[str, torch.Tensor]:
    """The float32 buffers GaussianDiffusion registers (sd:1056-1134), from the float64 betas of the named schedule.
    A beta >= 1 (the linear schedule below 21 timesteps) makes alphas_cumprod <= 0 and every chain NaN: the reference samples
    on in silence, this raises."""
    betas, ac = _schedule64(timesteps, beta_schedule)
    alphas = 1.0 - betas
    ac_prev = torch.nn.functional.pad(ac[:-1], (1, 0), value=1.0)
    post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
    buf = {
        "betas": betas, "alphas_cumprod": ac, "alphas_cumprod_prev": ac_prev,
        "sqrt_alphas_cumprod": torch.sqrt(ac), "sqrt_one_minus_alphas_cumprod": torch.sqrt(1.0 - ac),
        "log_one_minus_alphas_cumprod": torch.log(1.0 - ac), "sqrt_recip_alphas_cumprod": torch.sqrt(1.0 / ac),
        "sqrt_recipm1_alphas_cumprod": torch.sqrt(1.0 / ac - 1), "posterior_variance": post_var,
        "posterior_log_variance_clipped": torch.log(post_var.clamp(min=1e-20)),
        "posterior_mean_coef1": betas * torch.sqrt(ac_prev) / (1.0 - ac),
        "posterior_mean_coef2": (1.0 - ac_prev) * torch.sqrt(alphas) / (1.0 - ac),
        "loss_weight": ac / (1 - ac),
    }
    return {k: v.to(torch.float32) for k, v in buf.items()}


def loss_weight(timesteps: int, beta_schedule: str, objective: str, min_snr_loss_weight: bool = False,
                min_snr_gamma=5) -> torch.Tensor:
    """The reference's per-timestep loss weight of an objective (sd:1138-1151): computed in float64 from the signal-to-noise
    ratio alphas_cumprod / (1 - alphas_cumprod), clipped at min_snr_gamma on request, stored as float32."""
    _betas, ac = _schedule64(timesteps, beta_schedule)
    snr = ac / (1 - ac)
    clipped = snr.clone()
    if min_snr_loss_weight:
        clipped.clamp_(max=min_snr_gamma)
    if objective == "pred_noise":
        w = clipped / snr
    elif objective == "pred_x0":
        w = clipped
    elif objective == "pred_v":
        w = clipped / (snr + 1)
    else:
        raise ValueError(f"unknown objective {objective}")
    return w.to(torch.float32)


def ddim_times(total: int, steps: int) -> List[int]:
    """[T-1, ..., -1]: linspace(-1, T-1, steps+1) truncated to int, reversed (sd:1331-1334)."""
    return list(reversed(torch.linspace(-1, total - 1, steps=steps + 1).int().tolist()))



class _ProfileShape(C.Structure):     # include/prg.h: prg_profile_shape
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32), ("ups", C.c_int32),
                ("hout", C.c_int32), ("wout", C.c_int32), ("two_source", C.c_int32), ("prologue", C.c_int32),
                ("mx", C.c_int32), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double), ("flops_executed", C.c_double)]

class GaussianDiffusion:
    """Sampling half of the reference class: same constructor keywords, ``sample(param_cond=, img_cond=)``.

    ``objective`` and ``beta_schedule``: left out, they are the generator's ``pred_x0`` / ``sigmoid`` (generate_dataset.py:34-44).
    Any other configuration names BOTH.  The reference class defaults to ``pred_noise`` / ``cosine``, so a call that names one
    of them and leaves the other to a default means one model there and another here (``objective='pred_noise'`` alone: cosine
    in the reference, sigmoid here); it is refused with ``ValueError`` instead of sampling from the wrong schedule in silence."""

    def __init__(self, model: Unet, *, image_size, timesteps=1000, sampling_timesteps=None, loss_type="l1",
                 objective=None, beta_schedule=None, ddim_sampling_eta=1.0, min_snr_loss_weight=False, min_snr_gamma=5,
                 is_ddnm_sampling=True, ddnm_sampling_dropout=0.0, ddnm_dropout_schedule="none"):
        given = (objective is not None, beta_schedule is not None)
        objective = "pred_x0" if objective is None else objective
        beta_schedule = "sigmoid" if beta_schedule is None else beta_schedule
        if given != (True, True) and (objective, beta_schedule) != ("pred_x0", "sigmoid"):
            raise ValueError(f"objective='{objective}', beta_schedule='{beta_schedule}': a configuration other than the generator's "
                             "pred_x0 / sigmoid names both keywords (the reference class's defaults are pred_noise / cosine, "
                             "not this project's: the one left out would not mean what it means there)")
        if objective not in OBJECTIVES:
            raise ValueError(f"unknown objective {objective}: one of {', '.join(OBJECTIVES)}")
        if beta_schedule not in BETA_SCHEDULES:
            raise ValueError(f"unknown beta schedule {beta_schedule}: one of {', '.join(BETA_SCHEDULES)}")
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"invalid loss type {loss_type}: one of {', '.join(LOSS_TYPES)}")
        if not 0.0 <= float(ddnm_sampling_dropout) <= 1.0:
            raise ValueError(f"ddnm_sampling_dropout must lie in [0, 1], got {ddnm_sampling_dropout}")
        if ddnm_dropout_schedule not in ("none", "linear"):
            raise ValueError(f"unknown ddnm dropout schedule {ddnm_dropout_schedule}")
        assert not model.random_or_learned_sinusoidal_cond and model.channels == model.out_dim
        self.model, self.channels, self.image_size = model, model.channels, int(image_size)
        self.objective, self.is_ddnm_sampling = objective, bool(is_ddnm_sampling)
        self.num_timesteps = int(timesteps)
        self.sampling_timesteps = int(sampling_timesteps) if sampling_timesteps is not None else int(timesteps)
        assert self.sampling_timesteps <= self.num_timesteps
        self.is_ddim_sampling = self.sampling_timesteps < self.num_timesteps
        self.ddim_sampling_eta = float(ddim_sampling_eta)
        self.beta_schedule = beta_schedule
        for k, v in make_schedule(self.num_timesteps, beta_schedule).items():
            setattr(self, k, v)
        # the training objective's weight (sd:1138-1151); pred_x0 without the min-SNR clip is make_schedule's own entry
        self.loss_type = loss_type
        self.min_snr_loss_weight, self.min_snr_gamma = bool(min_snr_loss_weight), min_snr_gamma
        self.loss_weight = loss_weight(self.num_timesteps, beta_schedule, objective, self.min_snr_loss_weight, min_snr_gamma)
        # the refine row of the ancestral sampler is p_sample(t = 0) whose posterior mean the kernel takes to be x0 itself
        # (sd:1173-1176, 1307-1314): true of the schedule built here, not assumed of every schedule
        assert float(self.posterior_mean_coef1[0]) == 1.0 and float(self.posterior_mean_coef2[0]) == 0.0, \
            f"beta_schedule='{beta_schedule}', timesteps={timesteps}: posterior_mean_coef1[0], coef2[0] are not 1, 0 in float32"
        # stochastic DDNM (sd:1075-1094): per-timestep probability of NOT replacing a known pixel, float64 like the reference's
        self.ddnm_sampling_dropout = float(ddnm_sampling_dropout)
        self.ddnm_dropout_schedule = ddnm_dropout_schedule
        self.ddnm_dropouts = torch.linspace(self.ddnm_sampling_dropout,
                                            self.ddnm_sampling_dropout if ddnm_dropout_schedule == "none" else 0.0,
                                            self.num_timesteps, dtype=torch.float64)
        self.denoise_dropouts = torch.linspace(1.0, 0.0, self.num_timesteps, dtype=torch.float64) ** 100
        self._samplers = {}            # (batch, size, refine, mode) -> (handle, whether its keep table has a drawing row)
        dep = getattr(model, "_dependents", None)
        if dep is not None:
            dep.add(self)               # reloading / closing the network drops the samplers built on its old handle

    # -- transition table -------------------------------------------------------------------------
    def step_table(self) -> List[dict]:
        """One dict per transition, in execution order; field meaning documented at prg_step (include/prg.h)."""
        rows = []
        if not self.is_ddim_sampling:                                   # p_sample_loop (sd:1283-1317)
            for t in reversed(range(self.num_timesteps)):
                sig = (0.5 * self.posterior_log_variance_clipped[t]).exp() if t > 0 else torch.tensor(0.0)
                rows.append(dict(t=t, clip_pred=2, c_x0=self.posterior_mean_coef1[t], c_x=self.posterior_mean_coef2[t],
                                 c_eps=0.0, sigma=sig, sqrt_recip=self.sqrt_recip_alphas_cumprod[t],
                                 sqrt_recipm1=self.sqrt_recipm1_alphas_cumprod[t]))
        else:                                                           # ddim_sample (sd:1319-1392)
            times = ddim_times(self.num_timesteps, self.sampling_timesteps)
            for t, tn in zip(times[:-1], times[1:]):
                row = dict(t=t, clip_pred=1, sqrt_recip=self.sqrt_recip_alphas_cumprod[t],
                           sqrt_recipm1=self.sqrt_recipm1_alphas_cumprod[t])
                if tn < 0:
                    row.update(c_x0=1.0, c_x=0.0, c_eps=0.0, sigma=0.0)
                else:
                    a, an = self.alphas_cumprod[t], self.alphas_cumprod[tn]
                    sigma = self.ddim_sampling_eta * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
                    c = (1 - an - sigma ** 2).sqrt()
                    row.update(c_x0=an.sqrt(), c_x=0.0, c_eps=c, sigma=sigma)
                rows.append(row)
        return [{k: (float(v) if k not in ("t", "clip_pred") else int(v)) for k, v in r.items()} for r in rows]

    def _steps_c(self, refine: bool = False):
        rows = self.step_table()
        if refine:
            # has_refine_step (sd:1307-1314 / sd:1374-1388): one more evaluation at t = 0 WITHOUT the DDNM replacement;
            # the known pixels take its clamped output, the in-painted ones keep their value
            rows = rows + [dict(t=0, clip_pred=4, c_x0=0.0, c_x=0.0, c_eps=0.0, sigma=0.0,
                                sqrt_recip=float(self.sqrt_recip_alphas_cumprod[0]),
                                sqrt_recipm1=float(self.sqrt_recipm1_alphas_cumprod[0]))]
        arr = (_lib.StepC * len(rows))()
        for i, r in enumerate(rows):
            arr[i] = _lib.StepC(r["t"], r["clip_pred"], r["c_x0"], r["c_x"], r["c_eps"], r["sigma"], r["sqrt_recip"],
                                r["sqrt_recipm1"])
        return arr, len(rows)

    def objective_table(self, refine: bool = False):
        """One (p, q) pair per row of ``_steps_c(refine)`` (prg_sampler_set_objective, include/prg.h): the row's x0 before the
        clamp is ``p * x - q * u``.  ``pred_noise``: (sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t]) (sd:1153-1156);
        ``pred_v``: (sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]) (sd:1169-1171); ``pred_x0``: None, u is x0."""
        if self.objective == "pred_x0":
            return None
        p, q = ((self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod) if self.objective == "pred_noise" else
                (self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod))
        ts = [r["t"] for r in self.step_table()] + ([0] if refine else [])
        return [(float(p[t]), float(q[t])) for t in ts]

    def _objective_c(self, refine: bool = False):
        """(code, p, q) for the C entries; the arrays are None for pred_x0."""
        tab = self.objective_table(refine)
        if tab is None:
            return 0, None, None
        return (OBJECTIVES[self.objective], (C.c_float * len(tab))(*[p for p, _q in tab]),
                (C.c_float * len(tab))(*[q for _p, q in tab]))

    def keep_table(self, mode: str = "sample", refine: bool = False) -> List[float]:
        """One keep threshold per row of ``_steps_c(refine)`` for a run WITH a condition (prg_sampler_set_keep, include/prg.h):
        >= 0: the row draws a uniform per pixel and replaces a known pixel iff ``u > threshold`` in float32; -1: it replaces
        every known pixel and draws nothing.  ``sample`` and, on an ``is_ddnm_sampling`` model, ``denoise`` (whose own branch
        is then never reached, sd:1210 / 1220): float32(ddnm_dropouts[t]) where that is > 0 in float64 -- the reference draws
        nothing at p = 0 (sd:1213).  ``denoise`` otherwise: float32(denoise_dropouts[t]), always a draw; many of these
        underflow to 0, which is still a draw (``u > 0``).  The refine row never draws (is_ban_ddnm, sd:1312 / 1386)."""
        if mode not in ("sample", "denoise"):
            raise ValueError(f"unknown sampler mode {mode}")
        keep = []
        for r in self.step_table():
            if self.is_ddnm_sampling:
                p = self.ddnm_dropouts[r["t"]]
                keep.append(float(p.to(torch.float32)) if p > 0 else -1.0)
            elif mode == "denoise":
                keep.append(float(self.denoise_dropouts[r["t"]].to(torch.float32)))
            else:
                keep.append(-1.0)
        return keep + ([-1.0] if refine else [])

    def _keep_c(self, mode: str = "sample", refine: bool = False):
        """The table as a C array, or None when no row draws: then none is set and the run is plain DDNM."""
        keep = self.keep_table(mode, refine)
        return (C.c_float * len(keep))(*keep) if any(k >= 0 for k in keep) else None

    @property
    def n_draws(self) -> int:
        """Noise slabs a stored-noise run consumes: the start image + one per transition that adds noise
        (every transition but the last, for both samplers) = the reference's number of randn draws."""
        rows = self.step_table()
        return 1 + max([k + 1 for k, r in enumerate(rows) if r["sigma"] != 0.0], default=0)

    def _sampler(self, batch: int, refine: bool = False, mode: str = "sample"):
        """One handle (and one captured graph) per mode: sample() and denoise() differ in their keep table."""
        key = (batch, self.image_size, bool(refine), mode)
        if key not in self._samplers:
            lib = _lib.load()
            arr, n = self._steps_c(refine)
            h = C.c_void_p()
            _lib.check(lib.prg_sampler_create(self.model.handle, arr, n, batch, self.image_size, C.byref(h)),
                       "prg_sampler_create")
            keep = self._keep_c(mode, refine)
            if keep is not None:
                _lib.check(lib.prg_sampler_set_keep(h, keep, n), "prg_sampler_set_keep")
            code, op, oq = self._objective_c(refine)
            if code:                    # independent of the keep table; pred_x0 sets nothing: the handle's default
                _lib.check(lib.prg_sampler_set_objective(h, code, op, oq, n), "prg_sampler_set_objective")
            self._samplers[key] = (h, keep is not None)
        return self._samplers[key][0]

    def close(self):
        lib = _lib.load()
        for h, _draws in self._samplers.values():
            lib.prg_sampler_destroy(h)
        self._samplers.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- sampling ---------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, *, param_cond: torch.Tensor, img_cond: Optional[torch.Tensor] = None, disable_tqdm=True,
               has_refine_step=False, noise: Optional[torch.Tensor] = None, seeds: Optional[Sequence[int]] = None,
               use_graph: bool = True, profile: bool = False, keep_draws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(B,4) intrinsics vector, (B,2,S,S) condition in [-1,1] -> (B,1,S,S) depth in [0,1]  (sd:1394-1409).

        ``noise``: (n_draws,B,1,S,S) stored draws in the reference's order (parity runs); otherwise on-device
        Philox keyed by ``seeds`` (one 64-bit key per scene, default 0..B-1).  With ``ddnm_sampling_dropout`` > 0 every
        transition whose ``keep_table`` entry is >= 0 thins the known pixels out with a keep mask (sd:1213-1216):
        ``keep_draws`` (rows,B,1,S,S) stored uniforms, slab k for transition k, read only where the entry is >= 0 (parity
        runs); otherwise on-device Philox keyed by the same ``seeds``."""
        return self._run("sample", param_cond, img_cond, has_refine_step, noise, seeds, use_graph, profile, keep_draws)

    @torch.no_grad()
    def denoise(self, *, param_cond: torch.Tensor, img_cond: Optional[torch.Tensor] = None, disable_tqdm=True,
                has_refine_step=False, noise: Optional[torch.Tensor] = None, seeds: Optional[Sequence[int]] = None,
                use_graph: bool = True, profile: bool = False, keep_draws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``sample`` with is_denoise=True (sd:1411-1427): on a model with ``is_ddnm_sampling=False`` every transition replaces
        the known pixels it keeps under ``denoise_dropouts`` (sd:1220-1227), so the condition reaches the device there too;
        on an ``is_ddnm_sampling`` model it is ``sample``."""
        return self._run("denoise", param_cond, img_cond, has_refine_step, noise, seeds, use_graph, profile, keep_draws)

    def _run(self, mode, param_cond, img_cond, has_refine_step, noise, seeds, use_graph, profile, keep_draws):
        lib = _lib.load()
        pc = param_cond.to(device="cuda", dtype=torch.float32).contiguous()
        B, S = pc.shape[0], self.image_size
        cond = None
        if img_cond is not None and (self.is_ddnm_sampling or mode == "denoise"):
            cond = img_cond.to(device="cuda", dtype=torch.float32).contiguous()
            assert tuple(cond.shape) == (B, 2, S, S)
        refine = bool(has_refine_step) and cond is not None
        h = self._sampler(B, refine, mode)
        _lib.check(lib.prg_sampler_set_graph(h, int(use_graph)))
        _lib.check(lib.prg_sampler_set_profile(h, int(profile)))
        drawing = cond is not None and self._samplers[(B, S, refine, mode)][1]
        ku = None
        if keep_draws is not None and drawing:
            ku = keep_draws.to(device="cuda", dtype=torch.float32).contiguous()
            assert ku.numel() % (B * S * S) == 0, f"stored keep draws are slabs of shape ({B},1,{S},{S})"
        _lib.check(lib.prg_sampler_set_keep_draws(h, _lib.ptr(ku), 0 if ku is None else ku.numel() // (B * S * S)))
        nz = None
        seed_arr = None
        if noise is not None:
            nz = noise.to(device="cuda", dtype=torch.float32).contiguous()
            assert nz.numel() % (B * S * S) == 0 and nz.numel() // (B * S * S) >= self.n_draws, \
                f"stored noise needs {self.n_draws} draws of shape ({B},1,{S},{S})"
        if noise is None or (drawing and ku is None):
            seed_arr = (C.c_uint64 * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in (seeds if seeds is not None else range(B))])
        out = torch.empty((B, 1, S, S), dtype=torch.float32, device="cuda")
        _lib.check(lib.prg_sampler_run(h, _lib.ptr(pc), _lib.ptr(cond), _lib.ptr(nz),
                                       0 if nz is None else nz.numel() // (B * S * S),
                                       C.cast(seed_arr, C.c_void_p) if seed_arr is not None else None,
                                       _lib.ptr(out), _lib.stream_ptr()), "prg_sampler_run")
        self._keepalive = (pc, cond, nz, ku)   # the run is asynchronous: keep inputs alive until the next call
        return out

    # -- validation: the training objective on held-out images (sd:1448-1510) ------------------------
    def _val_q_sample(self, x0, a, s, noise, seeds, draw):
        from . import validate as V
        return V.q_sample_hip(x0, a.to(x0.device), s.to(x0.device), noise, seeds=seeds, draw=draw)

    def _val_loss(self, u, x0, a, s, w, noise, seeds, draw):
        from . import validate as V
        dev = x0.device
        return V.diffusion_loss_hip(u, x0, a.to(dev), s.to(dev), w.to(dev), self.objective, self.loss_type, noise, seeds=seeds, draw=draw)

    def _val_device(self):
        _lib.require_gpu()
        return torch.device("cuda", torch.cuda.current_device())

    def _val_inputs(self, x_start, t, noise, seeds):
        """x0 and the stored noise on the path's device, the timesteps on the host, and the per-sample coefficients gathered from
        the float32 buffers like the reference's extract() (sd:968-971)."""
        dev = self._val_device()
        x0 = torch.as_tensor(x_start).to(device=dev, dtype=torch.float32).contiguous()
        B = x0.shape[0]
        t = torch.as_tensor(t).to(device="cpu", dtype=torch.int64).reshape(-1)
        if t.shape[0] != B or int(t.min()) < 0 or int(t.max()) >= self.num_timesteps:
            raise ValueError(f"t: one timestep in [0, {self.num_timesteps}) per sample")
        if noise is not None and seeds is not None:
            raise ValueError("stored noise or Philox seeds, not both")
        nz = None
        if noise is not None:
            nz = torch.as_tensor(noise).to(device=dev, dtype=torch.float32).contiguous()
            assert nz.shape == x0.shape, "noise has x_start's shape"
        elif seeds is None:
            seeds = range(B)                                  # sample()'s default keys
        return x0, t, nz, (None if nz is not None else list(seeds)), self.sqrt_alphas_cumprod[t], self.sqrt_one_minus_alphas_cumprod[t]

    @torch.no_grad()
    def q_sample(self, x_start, t, noise=None, *, seeds=None, draw=0):
        """x_t = sqrt_alphas_cumprod[t] x_start + sqrt_one_minus_alphas_cumprod[t] noise (sd:1448-1453), prg_q_sample.  ``noise``:
        stored normals of x_start's shape; otherwise on-device Philox keyed per sample by ``seeds`` (default 0..B-1) at draw
        index ``draw``, under the validation path's own stream tag: no draw is shared with a chain of the same seeds."""
        x0, _t, nz, seeds, a, s = self._val_inputs(x_start, t, noise, seeds)
        return self._val_q_sample(x0, a, s, nz, seeds, draw)

    @torch.no_grad()
    def p_losses(self, x_start, t, param_cond, *, noise=None, seeds=None, draw=0, per_sample=False):
        """The training loss of x_start (B,1,S,S) in [-1,1] at the timesteps t (B,) (sd:1464-1497): prg_q_sample -> Unet.forward ->
        prg_diffusion_loss.  With Philox noise the noise is never stored: the loss kernel draws it again.  Returns the batch mean
        of the weighted losses (float64, 0-dim); ``per_sample=True``: the (B,2) float64 table [unweighted mean, weighted loss]."""
        x0, t, nz, seeds, a, s = self._val_inputs(x_start, t, noise, seeds)
        x_t = self._val_q_sample(x0, a, s, nz, seeds, draw)
        u = self.model(x_t, t.to(x_t.device), torch.as_tensor(param_cond).to(device=x_t.device, dtype=torch.float32))
        table = self._val_loss(u, x0, a, s, self.loss_weight[t], nz, seeds, draw)
        return table if per_sample else table[:, 1].mean()

    def forward(self, data_dict, *, seed=0, draw=0, **kwargs):
        """The reference's forward (sd:1499-1510) with keyed draws: ``img`` (B,1,S,S) in [0,1] normalised to [-1,1], ``intrinsic``
        (B,3,3) -> param_vector; the timesteps are ``validate.timesteps(seed, scenes, draw, T)`` and, unless the caller passes
        noise or seeds, the noise keys ``synthetic.noise_seed(seed, scene)``, with scenes = data_dict["scene"] (default 0..B-1):
        the same (seed, scene, draw) gives the same t and the same noise whatever the batch or the shard."""
        from . import geometry as G
        from . import synthetic, validate as V
        img = torch.as_tensor(data_dict["img"])
        B, _c, h, w = img.shape
        assert h == self.image_size and w == self.image_size, f"height and width of image must be {self.image_size}"
        scenes = [int(i) for i in data_dict.get("scene", range(B))]
        t = torch.from_numpy(V.timesteps(seed, scenes, draw, self.num_timesteps))
        if kwargs.get("noise") is None and kwargs.get("seeds") is None:
            kwargs["seeds"] = [synthetic.noise_seed(seed, i) for i in scenes]
        return self.p_losses(img.to(torch.float32) * 2 - 1, t, G.param_vector(torch.as_tensor(data_dict["intrinsic"])), draw=draw, **kwargs)

    def last_profile(self, batch: int, refine: bool = False) -> dict:
        lib = _lib.load()
        h = self._sampler(batch, refine)
        ms, n, fl, tot = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        _lib.check(lib.prg_sampler_get_profile(h, C.byref(ms), C.byref(n), C.byref(fl), C.byref(tot)))
        by = C.c_double()
        _lib.check(lib.prg_sampler_get_profile_bytes(h, C.byref(by)))
        sms, sn = C.c_double(), C.c_int64()
        _lib.check(lib.prg_sampler_get_profile_step(h, C.byref(sms), C.byref(sn)))
        ex = C.c_double()
        _lib.check(lib.prg_sampler_get_profile_executed(h, C.byref(ex)))
        nrows = C.c_int32()
        _lib.check(lib.prg_sampler_get_profile_shapes(h, None, 0, C.byref(nrows)))
        rows = (_ProfileShape * max(1, nrows.value))()
        _lib.check(lib.prg_sampler_get_profile_shapes(h, C.cast(rows, C.c_void_p), nrows.value, C.byref(nrows)))
        shapes = [{f: getattr(rows[i], f) for f, _ in _ProfileShape._fields_} for i in range(nrows.value)]
        return {"conv_ms": ms.value, "conv_launches": n.value, "conv_flops": fl.value, "conv_bytes": by.value, "conv_flops_executed": ex.value,
                "total_ms": tot.value, "step_ms": sms.value, "step_launches": sn.value, "conv_shapes": shapes}
