"""Checkpoint validation: what a checkpoint's training objective is on held-out depth maps, per timestep and per storage mode,
and the depth-correction network's evaluation metrics.

The reference answers both with short code paths: ``GaussianDiffusion.forward`` / ``p_losses`` / ``q_sample`` (sd:1448-1510)
and ``MaskTrainer.compute_metrics`` (dc:1229-1275).  On the device they are three streaming kernels (csrc/validate.hip,
include/prg.h): ``prg_q_sample``, ``prg_diffusion_loss``, ``prg_mask_metrics``.  This module holds

  * their numpy specifications (``q_sample_spec``, ``diffusion_loss_spec``, ``mask_metrics_spec``): the same float32 steps and
    the same float64 summation order (``ordered_sum``), bit-identical to the kernels on stored noise, and the ``device="cpu"``
    path together with ``prg_cpu_unet_forward``;
  * ``mask_metrics``: the reference's six numbers from a batch's sums, and ``MetricMeter``, its running average;
  * ``timesteps``: a keyed timestep draw, a pure function of (seed, scene, draw, T);
  * ``loss_profile``: every image at every listed timestep, one U-Net evaluation per (image, timestep).

sd = denoising_diffusion_pytorch/successive_ddnm_diffusion.py, dc = depth_correction_pytorch/depth_correction.py of the reference.
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from .philox import philox4x32_10

BLOCK_PIXELS = 4096                 # pixels per workgroup of the kernels: 256 threads x 4 quads x 4 pixels
TAG_NOISE = 0x76616C64              # "vald": third Philox counter word of the forward process' normals (csrc/sampler.h)
TAG_TIMESTEP = 0x7674696D           # "vtim": of the timestep draw
OBJECTIVES = {"pred_x0": 0, "pred_noise": 1, "pred_v": 2}
LOSS_TYPES = {"l1": 0, "l2": 1}
LABEL_TOL = 0.005                   # PairedDepthDataset's label mask: |label - input| < 0.005 (dc:941)


# ----------------------------------------------------------------------------------------------------------------------
# the summation order
# ----------------------------------------------------------------------------------------------------------------------
def ordered_sum(terms) -> np.ndarray:
    """(B, HW) float32 terms -> (B,) float64 sums in the kernels' order, which depends on HW alone (csrc/validate.hip):
    the row is cut into blocks of 4096 pixels; thread j of 256 adds the terms of its quads j, j + 256, j + 512, j + 768 one by
    one in pixel order to a float64 accumulator starting at +0; six pairwise folds over neighbouring lanes give each of the
    four wave totals; these are added in wave order; the block partials are added in index order.  Pixels past HW add +0."""
    t = np.asarray(terms, dtype=np.float32)
    assert t.ndim == 2
    B, HW = t.shape
    nblk = -(-HW // BLOCK_PIXELS)
    p = np.zeros((B, nblk * BLOCK_PIXELS), dtype=np.float64)
    p[:, :HW] = t
    p = p.reshape(B, nblk, 4, 256, 4)                   # block, quad of the thread, thread, pixel of the quad
    acc = np.zeros((B, nblk, 256), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for it in range(4):
            for e in range(4):
                acc = acc + p[:, :, it, :, e]
        v = acc.reshape(B, nblk, 4, 64)
        for _ in range(6):
            v = v[..., 0::2] + v[..., 1::2]
        w = v[..., 0]
        blk = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
        s = np.zeros(B, dtype=np.float64)
        for k in range(nblk):
            s = s + blk[:, k]
    return s


def _rows(x, B=None) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    return a.reshape(a.shape[0] if B is None else B, -1)


# ----------------------------------------------------------------------------------------------------------------------
# numpy specifications of the three kernels
# ----------------------------------------------------------------------------------------------------------------------
def q_sample_spec(x0, a, s, noise) -> np.ndarray:
    """x_t = fl(fl(a x0) + fl(s n)) per sample: two rounded float32 products and one addition (sd:1451-1453).  x0, noise
    (B, ...) float32; a, s (B,) float32.  Returns x0's shape."""
    x, n = _rows(x0), _rows(noise)
    a = np.asarray(a, dtype=np.float32).reshape(-1, 1)
    s = np.asarray(s, dtype=np.float32).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((a * x) + (s * n)).astype(np.float32).reshape(np.shape(x0))


def predict_v_spec(x0, a, s, noise) -> np.ndarray:
    """The pred_v target fl(fl(a n) - fl(s x0)) (sd:1164-1167)."""
    x, n = _rows(x0), _rows(noise)
    a = np.asarray(a, dtype=np.float32).reshape(-1, 1)
    s = np.asarray(s, dtype=np.float32).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((a * n) - (s * x)).astype(np.float32).reshape(np.shape(x0))


def diffusion_loss_spec(u, x0, noise, a, s, w, objective, loss_type) -> np.ndarray:
    """prg_diffusion_loss in numpy -> (B, 2) float64: the unweighted mean and mean * (double)w.  objective / loss_type: the names
    or the codes of include/prg.h.  noise may be None for pred_x0."""
    objective = OBJECTIVES.get(objective, objective)
    loss_type = LOSS_TYPES.get(loss_type, loss_type)
    if objective not in (0, 1, 2) or loss_type not in (0, 1):
        raise ValueError("unknown objective or loss type")
    uu, x = _rows(u), _rows(x0)
    B, HW = x.shape
    if objective == 0:
        target = x
    elif objective == 1:
        target = _rows(noise)
    else:
        target = _rows(predict_v_spec(x, a, s, _rows(noise)))
    with np.errstate(invalid="ignore", over="ignore"):
        d = (uu - target).astype(np.float32)
        term = np.abs(d) if loss_type == 0 else (d * d).astype(np.float32)
        mean = ordered_sum(term) / np.float64(HW)
        return np.stack([mean, mean * np.asarray(w, dtype=np.float32).astype(np.float64).reshape(-1)], axis=1)


def mask_metrics_spec(prob, input, label, mask=None, threshold=0.5, tol=LABEL_TOL):
    """prg_mask_metrics in numpy -> (counts (B, 4) int64 at index 2 m + o, sums (B, 2) float64 of |d| and fl(d d))."""
    p, i, l = _rows(prob), _rows(input), _rows(label)
    thr = np.float32(threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        mv = _rows(mask) if mask is not None else (np.abs((l - i).astype(np.float32)) < np.float32(tol)).astype(np.float32)
        o, m = p > thr, mv > thr                                   # NaN and a value at the threshold: False
        out = np.where(o, i, np.float32(0)).astype(np.float32)
        lab = np.where(m, l, np.float32(0)).astype(np.float32)
        d = (lab - out).astype(np.float32)
        idx = 2 * m.astype(np.int64) + o.astype(np.int64)
        counts = np.stack([(idx == k).sum(axis=1) for k in range(4)], axis=1).astype(np.int64)
        sums = np.stack([ordered_sum(np.abs(d)), ordered_sum((d * d).astype(np.float32))], axis=1)
    return counts, sums


# ----------------------------------------------------------------------------------------------------------------------
# compute_metrics' numbers from the sums
# ----------------------------------------------------------------------------------------------------------------------
def mask_metrics(sums) -> Dict[str, float]:
    """(counts (B, 4), sums (B, 2)) of ONE batch, HW implied by the counts -> the reference's numbers, formula for formula
    (dc:1240-1250): MSE / MAE = the batch's sums over its B HW pixels, SAE = the sum of |d|; matrix = the 2 x 2 bincount of
    2 label + output; IoU = diag / (row sums + column sums - diag), mIoU its nanmean (a class without a pixel in either mask is
    0 / 0 and skipped); PAcc = trace / total; FP = matrix[0][1].  Divisions in float64."""
    counts, s = sums
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    s = np.asarray(s, dtype=np.float64).reshape(-1, 2)
    matrix = counts.sum(axis=0).reshape(2, 2)
    n = int(matrix.sum())
    s_abs = s_sq = np.float64(0.0)
    for b in range(len(s)):                              # batch sums in sample order
        s_abs, s_sq = s_abs + s[b, 0], s_sq + s[b, 1]
    inter = np.diag(matrix).astype(np.float64)
    union = (matrix.sum(axis=1) + matrix.sum(axis=0)).astype(np.float64) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / union
    ok = ~np.isnan(iou)
    miou = float(iou[ok].sum() / ok.sum()) if ok.any() else float("nan")
    return {"MSE": float(s_sq / n), "MAE": float(s_abs / n), "SAE": float(s_abs), "mIoU": miou,
            "PAcc": float(inter.sum() / n), "FP": int(matrix[0, 1]), "matrix": matrix}


class MetricMeter:
    """The reference's AverageMeter (dc:104-124) over the batches of an evaluation, one per metric: update() with mask_metrics'
    dictionary, `avg` the mean of the batches' values (each batch counts once, as there)."""

    KEYS = ("MSE", "MAE", "SAE", "mIoU", "PAcc", "FP")

    def __init__(self):
        self.sum = {k: 0.0 for k in self.KEYS}
        self.count = 0

    def update(self, metrics: Dict[str, float]):
        for k in self.KEYS:
            self.sum[k] += float(metrics[k])
        self.count += 1

    @property
    def avg(self) -> Dict[str, float]:
        return {k: self.sum[k] / self.count for k in self.KEYS}


# ----------------------------------------------------------------------------------------------------------------------
# keyed draws
# ----------------------------------------------------------------------------------------------------------------------
def timesteps(seed: int, scenes, draw: int, T: int) -> np.ndarray:
    """One timestep in [0, T) per scene index: Philox4x32-10 under the key `seed` at counter {scene, draw, "vtim", 0}, first
    word w, t = (w T) >> 32.  A pure function of (seed, scene, draw, T): the same whatever the batch or the shard."""
    if not 1 <= int(T) < 2 ** 31:
        raise ValueError("T must lie in [1, 2^31)")
    sc = np.asarray(scenes, dtype=np.int64).reshape(-1)
    if sc.size and (sc.min() < 0 or sc.max() >= 2 ** 32):
        raise ValueError("scene indices must fit 32 bits")
    w = philox4x32_10(sc.astype(np.uint64), int(draw) & 0xFFFFFFFF, TAG_TIMESTEP, 0, seed)[0]
    return ((w.astype(np.uint64) * np.uint64(T)) >> np.uint64(32)).astype(np.int64)


def philox_normals(seeds: Sequence[int], draw: int, HW: int, tag: int = TAG_NOISE) -> np.ndarray:
    """The normals of prg_q_sample's Philox noise, (B, HW) float32, on the host: the same counters, words and float32 steps as
    csrc/philox.h's philox_normal4.  numpy's logf / sinf / cosf are not the device's: equal to a few ulp, not bit for bit (the
    CPU path's noise; the device path never stores its own)."""
    if HW % 4:
        raise ValueError("Philox noise needs H*W to be a multiple of 4")
    q = np.arange(HW // 4, dtype=np.uint64)
    k = np.float32(2.0 ** -32)
    out = np.empty((len(seeds), HW // 4, 4), dtype=np.float32)
    for b, seed in enumerate(seeds):
        c = philox4x32_10(q, int(draw) & 0xFFFFFFFF, tag, 0, seed)
        u0, u1, u2, u3 = ((w.astype(np.float32) + np.float32(0.5)) * k for w in c)
        r0 = np.sqrt(np.float32(-2.0) * np.log(np.clip(u0, np.float32(1e-12), np.float32(1.0))))
        r1 = np.sqrt(np.float32(-2.0) * np.log(np.clip(u2, np.float32(1e-12), np.float32(1.0))))
        a0, a1 = np.float32(6.283185307179586) * u1, np.float32(6.283185307179586) * u3
        out[b] = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)
    return out.reshape(len(seeds), HW)


# ----------------------------------------------------------------------------------------------------------------------
# device front-ends of the three entries (torch tensors on a HIP device)
# ----------------------------------------------------------------------------------------------------------------------
def _dev(t, dtype=None):
    import torch
    from . import _lib
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.PrgError("the validation kernels take tensors on a HIP device (device='cpu' is the numpy specification)")
    return t.contiguous() if dtype is None else t.to(dtype).contiguous()


def _seed_tensor(seeds, B, device):
    import torch
    arr = np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64)
    if arr.shape != (B,):
        raise ValueError(f"seeds: one key per sample, {B} of them")
    return torch.from_numpy(arr.view(np.int64)).to(device)


def _workspace(B, HW, device):
    import torch
    from . import _lib
    n = _lib.load().prg_validate_workspace_bytes(B, HW)
    if n == 0:
        raise _lib.PrgError(f"validation kernels: B = {B}, HW = {HW} out of range")
    return torch.empty(n // 8, dtype=torch.float64, device=device), n


def q_sample_hip(x0, a, s, noise=None, *, seeds=None, draw=0, want_noise=False):
    """prg_q_sample on device tensors: x0 (B, ...) float32, a, s (B,) float32 -> x_t (and the normals with want_noise)."""
    import torch
    from . import _lib
    lib = _lib.load()
    x0 = _dev(x0, torch.float32)
    B = x0.shape[0]
    HW = x0.numel() // B
    nz = _dev(noise, torch.float32) if noise is not None else None
    sd = _seed_tensor(seeds, B, x0.device) if seeds is not None else None
    a, s = _dev(a, torch.float32), _dev(s, torch.float32)
    x_t = torch.empty_like(x0)
    n_out = torch.empty_like(x0) if want_noise else None
    _lib.check(lib.prg_q_sample(_lib.ptr(x0), _lib.ptr(a), _lib.ptr(s), _lib.ptr(nz), _lib.ptr(sd), int(draw) & 0xFFFFFFFF, B, HW,
                                _lib.ptr(x_t), _lib.ptr(n_out), _lib.stream_ptr()), "prg_q_sample")
    return (x_t, n_out) if want_noise else x_t


def diffusion_loss_hip(u, x0, a, s, w, objective, loss_type, noise=None, *, seeds=None, draw=0):
    """prg_diffusion_loss on device tensors -> (B, 2) float64 device tensor."""
    import torch
    from . import _lib
    lib = _lib.load()
    u, x0 = _dev(u, torch.float32), _dev(x0, torch.float32)
    B = x0.shape[0]
    HW = x0.numel() // B
    nz = _dev(noise, torch.float32) if noise is not None else None
    sd = _seed_tensor(seeds, B, x0.device) if seeds is not None else None
    a, s, w = _dev(a, torch.float32), _dev(s, torch.float32), _dev(w, torch.float32)
    ws, nbytes = _workspace(B, HW, x0.device)
    out = torch.empty((B, 2), dtype=torch.float64, device=x0.device)
    _lib.check(lib.prg_diffusion_loss(_lib.ptr(u), _lib.ptr(x0), _lib.ptr(nz), _lib.ptr(sd), int(draw) & 0xFFFFFFFF, _lib.ptr(a),
                                      _lib.ptr(s), _lib.ptr(w), OBJECTIVES.get(objective, objective), LOSS_TYPES.get(loss_type, loss_type),
                                      B, HW, _lib.ptr(ws), nbytes, _lib.ptr(out), _lib.stream_ptr()), "prg_diffusion_loss")
    return out


def mask_metrics_hip(prob, input, label, mask=None, threshold=0.5, tol=LABEL_TOL):
    """prg_mask_metrics on device tensors -> (counts (B, 4) int64, sums (B, 2) float64) device tensors."""
    import torch
    from . import _lib
    lib = _lib.load()
    prob, input, label = _dev(prob, torch.float32), _dev(input, torch.float32), _dev(label, torch.float32)
    B = prob.shape[0]
    HW = prob.numel() // B
    mk = _dev(mask, torch.float32) if mask is not None else None
    ws, nbytes = _workspace(B, HW, prob.device)
    counts = torch.empty((B, 4), dtype=torch.int64, device=prob.device)
    sums = torch.empty((B, 2), dtype=torch.float64, device=prob.device)
    _lib.check(lib.prg_mask_metrics(_lib.ptr(prob), _lib.ptr(input), _lib.ptr(label), _lib.ptr(mk), float(threshold), float(tol), B, HW,
                                    _lib.ptr(ws), nbytes, _lib.ptr(counts), _lib.ptr(sums), _lib.stream_ptr()), "prg_mask_metrics")
    return counts, sums


def evaluate_mask(net, input, label, mask=None, threshold=0.5, tol=LABEL_TOL) -> Dict[str, float]:
    """compute_metrics of one batch: the depth-correction network's probability of `input` (B,1,S,S) against `label` (and its
    mask, default PairedDepthDataset's rule).  Device tensors run prg_mask_metrics, host tensors the specification."""
    import torch
    input, label = torch.as_tensor(input, dtype=torch.float32), torch.as_tensor(label, dtype=torch.float32)
    prob = net(input)
    if input.is_cuda:
        counts, sums = mask_metrics_hip(prob, input, label, mask, threshold, tol)
        return mask_metrics((counts.cpu().numpy(), sums.cpu().numpy()))
    return mask_metrics(mask_metrics_spec(prob.numpy(), input.numpy(), label.numpy(), None if mask is None else np.asarray(mask),
                                          threshold, tol))


# ----------------------------------------------------------------------------------------------------------------------
# loss per timestep
# ----------------------------------------------------------------------------------------------------------------------
def loss_profile(diffusion, depth, K, *, timesteps: Sequence[int], seeds: Sequence[int]) -> np.ndarray:
    """Every image at every listed timestep -> (len(timesteps), B, 2) float64: [..., 0] the unweighted mean loss, [..., 1] the
    weighted one.  depth (B,1,S,S) in [0,1] (normalised to [-1,1] like GaussianDiffusion.forward), K (B,3,3) intrinsics.
    The noise of image b is Philox under its own key seeds[b] (one per scene: `synthetic.noise_seed(seed, scene)`); the draw
    index is the position in the list, so two storage modes, batches or shards see the same noise for the same (scene, entry)."""
    import torch
    from . import geometry as G
    depth = torch.as_tensor(depth, dtype=torch.float32)
    B = depth.shape[0]
    x0 = depth * 2 - 1
    pc = G.param_vector(torch.as_tensor(K))
    rows = []
    for i, t in enumerate(timesteps):
        if not 0 <= int(t) < diffusion.num_timesteps:
            raise ValueError(f"timestep {t} outside [0, {diffusion.num_timesteps})")
        tt = torch.full((B,), int(t), dtype=torch.int64)
        rows.append(diffusion.p_losses(x0, tt, pc, seeds=seeds, draw=i, per_sample=True).cpu().numpy())
    return np.stack(rows) if rows else np.zeros((0, B, 2))
