"""Camera geometry of the generative data path: host-side mirror of the reference helpers.

Same names, argument meaning and error behaviour as the reference functions (cited per function,
sd = /root/reference/denoising_diffusion_pytorch/successive_ddnm_diffusion.py); the tensor ops run as HIP
kernels through the C-ABI (include/prg.h).  Tiny per-scene scalars (intrinsics, poses) stay on the host in
numpy exactly like the reference.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from scipy.spatial.transform import Rotation

from . import _lib

DEPTH_UNIT_M = 10.0   # normalised depth 1.0 == 10 m (sd:2458, sd:2552)
K_CANDIDATES_F = (585.0, 572.0, 583.0, 540.021232, 570.342205, 533.069214)   # sd:358-366
K_WEIGHTS = (7, 8, 18, 5, 47, 5)                                             # sd:367


# ------------------------------------------------------------------------------------------------
# host helpers (numpy)
# ------------------------------------------------------------------------------------------------

def candidate_intrinsics() -> np.ndarray:
    out = np.zeros((len(K_CANDIDATES_F), 3, 3), dtype=np.float32)
    out[:, 0, 0] = out[:, 1, 1] = np.asarray(K_CANDIDATES_F, dtype=np.float32)
    out[:, 0, 2], out[:, 1, 2], out[:, 2, 2] = 320.0, 240.0, 1.0
    return out


def random_sample_intrinsic(batch_size: int) -> np.ndarray:
    """One of the six 3DMatch intrinsics per item, numpy legacy RNG (sd:354-374)."""
    p = np.asarray(K_WEIGHTS, dtype=np.float64)
    idx = np.random.choice(len(K_CANDIDATES_F), batch_size, replace=True, p=p / p.sum())
    return candidate_intrinsics()[idx]


def intrinsic_transform(intrinsic: np.ndarray, resize: Optional[int] = None,
                        centercrop: Optional[int] = None) -> np.ndarray:
    """Intrinsics after Resize(int) + CenterCrop(int) (sd:47-119; int arguments, the form sd:2436-2441 uses)."""
    K = np.asarray(intrinsic)
    fx, fy, cx, cy = K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]
    size_x, size_y = np.int32(cx * 2), np.int32(cy * 2)
    new_x, new_y = size_x, size_y
    nfx, nfy, ncx, ncy = fx, fy, cx, cx   # (sic) the reference seeds new_cy with old_cx when resize is None (sd:67)
    if resize is not None:
        if not isinstance(resize, (int, np.integer)):
            raise TypeError("only integer resize is supported on this path")
        if (size_x < size_y).all():
            new_x, new_y = int(resize), np.int32(np.floor(resize * size_y / size_x))
        else:
            new_x, new_y = np.int32(np.floor(resize * size_x / size_y)), np.int32(resize)
        nfx, nfy = np.float32(fx * new_x / size_x), np.float32(fy * new_y / size_y)
        ncx, ncy = np.float32(new_x / 2), np.float32(new_y / 2)
    if centercrop is not None:
        if not isinstance(centercrop, (int, np.integer)):
            raise TypeError("only integer centercrop is supported on this path")
        ncx = ncx - np.int32(np.round((new_x - centercrop) / 2.0))
        ncy = ncy - np.int32(np.round((new_y - centercrop) / 2.0))
    out = np.zeros_like(K)
    out[..., 0, 0], out[..., 1, 1], out[..., 0, 2], out[..., 1, 2], out[..., 2, 2] = nfx, nfy, ncx, ncy, 1.0
    return out


def param_vector(intrinsic: torch.Tensor) -> torch.Tensor:
    """(…,3,3) -> (…,4) [fx, fy, cx, cy]  (sd:343-351)."""
    return torch.stack([intrinsic[..., 0, 0], intrinsic[..., 1, 1], intrinsic[..., 0, 2], intrinsic[..., 1, 2]], -1)


def random_sample_pose(batch_size: int, center=(0, 0, 3), rng=None) -> np.ndarray:
    """Random camera motion about a pivot 3 m ahead, numpy legacy RNG, same draw order (sd:417-443).  `rng`: a
    `np.random.RandomState` to draw from instead of numpy's process-wide legacy stream (same algorithm, same values)."""
    np_random = np.random if rng is None else rng
    theta = np_random.rand(batch_size) * (np.pi / 12) - np.pi / 24
    phi = np_random.rand(batch_size) * (np.pi / 6) - np.pi / 12
    rot = Rotation.from_euler("XYZ", np.stack((theta, phi, np.zeros(batch_size)), axis=-1)).as_matrix()
    c = np.array(center)
    jitter = np_random.randn(batch_size, 3) / 3
    jitter[:, -1] = 0
    T = np.stack([np.eye(4) for _ in range(batch_size)])
    T[:, :3, :3] = rot
    T[:, :3, 3] = c - rot @ c + jitter
    return T.astype(np.float32)


POSE_STREAM = 0x706F7365     # "pose": the word that keys the candidate streams apart from every other use of the seed
POSE_Z_TOL = 0.0375          # metres behind its pixel's nearest depth a row may lie and still count as seen (the occlusion filter's)


def pose_candidates(seed: int, scene: int, sample_idx: int, n: int, spread: float = 1.0) -> np.ndarray:
    """`n` candidate camera motions for view `sample_idx` of scene `scene` -> (n, 4, 4) float32.  `random_sample_pose`'s
    construction (sd:417-443: rotation about X then Y around a pivot 3 m ahead, xy jitter) with the two angle ranges (±7.5°,
    ±15°) and the jitter's σ (1/3 m) multiplied by `spread`; spread = 1 stays inside the reference's ranges.
    The draws come from `np.random.Generator(PCG64(SeedSequence([seed, scene, POSE_STREAM, sample_idx])))`, one stream per (scene,
    view), in this fixed order: per candidate theta (one uniform), phi (one uniform), then three normals (the third, z's, is drawn
    and dropped like the reference's).  So a scene's candidates depend on nothing but the four keys — not on the batch, the lane,
    the shard or a resume — and the first k of n candidates are the k candidates of a shorter list."""
    n = int(n)
    if n < 1 or not (np.isfinite(spread) and spread > 0):
        raise ValueError("pose_candidates: n >= 1 and a finite spread > 0")
    if min(int(seed), int(scene), int(sample_idx)) < 0:
        raise ValueError("pose_candidates: seed, scene and sample_idx must be >= 0")
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(scene), POSE_STREAM, int(sample_idx)])))
    theta, phi, jitter = np.empty(n), np.empty(n), np.empty((n, 3))
    for c in range(n):
        theta[c] = (rng.random() * (np.pi / 12) - np.pi / 24) * spread
        phi[c] = (rng.random() * (np.pi / 6) - np.pi / 12) * spread
        jitter[c] = rng.standard_normal(3) / 3 * spread
    jitter[:, -1] = 0
    rot = Rotation.from_euler("XYZ", np.stack((theta, phi, np.zeros(n)), axis=-1)).as_matrix()
    center = np.array((0, 0, 3))
    T = np.stack([np.eye(4) for _ in range(n)])
    T[:, :3, :3] = rot
    T[:, :3, 3] = center - rot @ center + jitter
    return T.astype(np.float32)


def select_pose_candidates(counts, rows: int, band) -> Tuple[int, float, bool]:
    """Which of one scene's candidates to generate: counts (N,3) integers (in_frame, seen, covered) as `pose_candidate_counts`
    returns them for the scene, rows = the rows of its source cloud, band = (lo, hi).  On the host, in float64: r_c = seen_c /
    rows; the FIRST c in index order with lo <= r_c <= hi wins; if none is in band, the c with the smallest max(lo - r_c, r_c - hi),
    ties to the lowest c; rows == 0 gives c = 0 (r = 0).  -> (c, r_c, in band)."""
    lo, hi = float(band[0]), float(band[1])
    seen = np.asarray(counts, dtype=np.int64).reshape(-1, 3)[:, 1].astype(np.float64)
    if len(seen) < 1:
        raise ValueError("select_pose_candidates: no candidate")
    if int(rows) <= 0:
        return 0, 0.0, bool(lo <= 0.0 <= hi)
    r = seen / np.float64(rows)
    inside = np.nonzero((r >= lo) & (r <= hi))[0]
    if len(inside):
        c = int(inside[0])
        return c, float(r[c]), True
    c = int(np.argmin(np.maximum(lo - r, r - hi)))          # argmin: the first of equal values
    return c, float(r[c]), False


def check_overlap_band(band) -> Tuple[float, float]:
    """(lo, hi) of an overlap target as floats; ValueError unless 0 <= lo < hi <= 1."""
    try:
        lo, hi = (float(v) for v in band)
    except (TypeError, ValueError):
        raise ValueError("overlap must be a pair (lo, hi)") from None
    if not 0.0 <= lo < hi <= 1.0:
        raise ValueError("overlap must satisfy 0 <= lo < hi <= 1")
    return lo, hi


# ------------------------------------------------------------------------------------------------
# device ops (HIP)
# ------------------------------------------------------------------------------------------------

def random_sample_transform(intrinsic: np.ndarray, image_size: int = 256) -> np.ndarray:
    """Random in-place camera rotation of Tester.generate (sd:377-415): pitch / yaw within the view frustum, any roll;
    translation drawn and multiplied by zero (the randn still consumes the legacy numpy stream).  float32 (B,4,4)."""
    K = np.asarray(intrinsic)
    batch = K.shape[0]
    h = w = image_size
    fx, fy, cx, cy = K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]
    th_min, th_max = -np.arctan((h - cy) / fy), np.arctan(cy / fy)
    ph_min, ph_max = -np.arctan(cx / fx), np.arctan((w - cx) / fx)
    theta = np.random.rand(batch) * (th_max - th_min) + th_min
    phi = np.random.rand(batch) * (ph_max - ph_min) + ph_min
    psi = np.random.rand(batch) * 2 * np.pi - np.pi
    R = Rotation.from_euler("XYZ", np.stack((theta, phi, psi), axis=-1), degrees=False).as_matrix()
    t = np.random.randn(batch, 3) / 3 * 0
    T = np.stack([np.eye(4) for _ in range(batch)])
    T[..., :3, :3] = R
    T[..., :3, 3] = t
    return T.astype(np.float32)


def _f32(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.PrgError("expected a tensor on the HIP device (this package has no CPU path)")
    return t.contiguous().to(torch.float32)


def _u8(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """bool (reinterpreted) or any other dtype (converted) -> flat contiguous uint8; None stays None."""
    if t is None:
        return None
    t = t.contiguous()
    return (t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)).view(-1)


def _dev_i32(a, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)


def _dev_i64(a, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)


def _ragged_f64(pts: torch.Tensor, offsets: torch.Tensor, n_pairs: Optional[int] = None):
    """What every ragged float64 function starts with: both tensors on the device, float64 / int64, contiguous, pts as
    (total,3); with `n_pairs`, offsets must be the 2*n_pairs+1 of a pair buffer.  -> (pts, offsets, total).  A buffer without
    rows comes back as one row of zeros, with total == 0: a tensor without elements has no address to pass."""
    if not (pts.is_cuda and offsets.is_cuda):
        raise _lib.PrgError("expected tensors on the HIP device (this package has no CPU path)")
    assert pts.dtype == torch.float64 and offsets.dtype == torch.int64
    assert n_pairs is None or offsets.numel() == 2 * int(n_pairs) + 1
    pts = pts.contiguous().view(-1, 3)
    total = pts.shape[0]
    if total == 0:
        pts = torch.zeros((1, 3), dtype=torch.float64, device=pts.device)
    return pts, offsets.contiguous(), total


def depth2pc_tensor(depth: torch.Tensor, intrinsic: torch.Tensor, *, clip=(0, 10), invalid_num=None):
    """(B,1,H,W) depth, (B,3,3) K -> pc (B,HW,3) (invalid -> NaN / invalid_num), valid (B,HW) bool  (sd:176-209)."""
    lib = _lib.load()
    depth, K = _f32(depth), _f32(intrinsic)
    B, Cc, H, W = depth.shape
    assert Cc == 1
    pc = torch.empty((B, H * W, 3), dtype=torch.float32, device=depth.device)
    valid = torch.empty((B, H * W), dtype=torch.uint8, device=depth.device)
    lo, hi = (1.0, 0.0) if clip is None else (float(clip[0]), float(clip[1]))
    inv = float("nan") if invalid_num is None else float(invalid_num)
    _lib.check(lib.prg_depth2pc(_lib.ptr(depth), _lib.ptr(K), _lib.ptr(pc), _lib.ptr(valid), B, H, W, lo, hi, inv,
                                _lib.stream_ptr()), "prg_depth2pc")
    return pc, valid.view(torch.bool)


def pc2depth_tensor(pc: torch.Tensor, valid: Optional[torch.Tensor], intrinsic: torch.Tensor, *,
                    image_size=(480, 640)):
    """Z-buffer: (B,N,3), (B,N) bool, (B,3,3) -> depth (B,1,H,W) f32 (nearest z, 0 = empty), mask bool  (sd:212-265)."""
    lib = _lib.load()
    pc, K = _f32(pc), _f32(intrinsic)
    B, N, _ = pc.shape
    H, W = int(image_size[0]), int(image_size[1])
    v8 = _u8(valid)
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=pc.device)
    mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=pc.device)
    _lib.check(lib.prg_pc2depth(_lib.ptr(pc), _lib.ptr(v8), _lib.ptr(K), _lib.ptr(depth), _lib.ptr(mask), B, N, H, W,
                                _lib.stream_ptr()), "prg_pc2depth")
    return depth, mask.view(torch.bool)


def reproject_tensor(depth: torch.Tensor, intrinsic: torch.Tensor, relative_pose: torch.Tensor, *, clip=(0, 10),
                     invalid_num=None, depth_unit: float = 1.0, out_scale: float = 1.0):
    """Unproject, move by the SE(3) pose, z-buffer into the same camera — one fused kernel (sd:268-286).

    ``depth_unit`` / ``out_scale`` fold the caller's `depth * 10` and `images_rpj * 0.1` (sd:484, sd:2552)."""
    lib = _lib.load()
    depth, K, P = _f32(depth), _f32(intrinsic), _f32(relative_pose)
    B, Cc, H, W = depth.shape
    assert Cc == 1 and clip is not None
    out = torch.empty_like(depth)
    mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=depth.device)
    _lib.check(lib.prg_reproject_zbuffer(_lib.ptr(depth), _lib.ptr(K), _lib.ptr(P), _lib.ptr(out), _lib.ptr(mask), B,
                                         H, W, float(depth_unit), float(clip[0]), float(clip[1]), float(out_scale),
                                         _lib.stream_ptr()), "prg_reproject_zbuffer")
    return out, mask.view(torch.bool)


def project_clouds(clouds: Sequence[np.ndarray], poses: np.ndarray, intrinsic: np.ndarray, image_size: int,
                   device, depth_scale: float = 1.0):
    """Generator.generate's per-scene projection (sd:2531-2552) for a whole batch in one launch: ragged float32
    clouds (n_b,3) each moved by its (4,4) pose and z-buffered with its K; returns depth*depth_scale and mask."""
    pts, d_offs = upload_clouds(clouds, device)
    return project_cloud_buffer(pts, d_offs, poses, intrinsic, image_size, depth_scale=depth_scale)


def upload_clouds(clouds: Sequence[np.ndarray], device, dtype=np.float32):
    """A list of (n_b,3) host clouds as ONE ragged device buffer: (pts (max(total,1),3) `dtype`, offsets (B+1) int64)."""
    B = len(clouds)
    offs = np.zeros(B + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = torch.from_numpy(np.concatenate([np.asarray(c, dtype=dtype).reshape(-1, 3) for c in clouds], 0)
                           if offs[-1] else np.zeros((1, 3), dtype)).to(device)
    return pts, torch.from_numpy(offs).to(device)


def project_cloud_buffer(pts: torch.Tensor, d_offs: torch.Tensor, poses: np.ndarray, intrinsic: np.ndarray,
                         image_size: int, depth_scale: float = 1.0):
    """`project_clouds` for a cloud that already lives on the device: pts (N,3) float32 ragged, d_offs (B+1) int64 CSR
    offsets, both device tensors (rows beyond d_offs[B] are not read).  Nothing but the poses and intrinsics is uploaded."""
    lib = _lib.load()
    device = pts.device
    assert pts.is_cuda and pts.dtype == torch.float32 and d_offs.dtype == torch.int64 and d_offs.device == device
    B = d_offs.numel() - 1
    P = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32)).to(device)
    K = torch.from_numpy(np.ascontiguousarray(intrinsic, dtype=np.float32)).to(device)
    S = int(image_size)
    depth = torch.empty((B, 1, S, S), dtype=torch.float32, device=device)
    mask = torch.empty((B, 1, S, S), dtype=torch.uint8, device=device)
    _lib.check(lib.prg_project_points_zbuffer(_lib.ptr(pts), _lib.ptr(d_offs), _lib.ptr(P), _lib.ptr(K), _lib.ptr(depth),
                                              _lib.ptr(mask), B, S, S, float(depth_scale), _lib.stream_ptr()),
               "prg_project_points_zbuffer")
    return depth, mask.view(torch.bool)


def _image_hw(S) -> Tuple[int, int]:
    """An image size as the generator passes it (one int, square) or as (H, W)."""
    if isinstance(S, (int, np.integer)):
        return int(S), int(S)
    H, W = S
    return int(H), int(W)


def _box6(box) -> Optional[np.ndarray]:
    """(lo, hi) -> the 6 float32 the scoring call reads on the host (lo xyz, hi xyz); None stays None."""
    if box is None:
        return None
    return np.concatenate([np.asarray(box[0], dtype=np.float32).reshape(3), np.asarray(box[1], dtype=np.float32).reshape(3)])


def pose_candidate_counts(pts: torch.Tensor, offs: torch.Tensor, poses, K, S, *, box=None, z_tol: float = POSE_Z_TOL,
                          workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """prg_pose_candidate_counts: N candidate poses per scene scored against the scene's cloud, which already lives on the device
    as `project_cloud_buffer` takes it (pts (rows,3) float32 ragged, offs (B+1) int64 CSR).  poses (B,N,4,4) and K (B,3,3):
    numpy or tensors (uploaded when on the host); S: the image size, an int or (H, W); box: (lo, hi) in the TARGET camera frame or
    None; z_tol in metres.  -> counts (B,N,3) int32 ON THE DEVICE: (in_frame, seen, covered) per candidate, bit for bit
    `postprocess.pose_candidate_counts` (which states the definition).  The workspace is a cached torch allocation of
    prg_pose_candidate_workspace_bytes, or of `workspace_bytes` when given (a smaller one makes the call chunk the candidates;
    the counts are the same).  Host synchronisations: none — the caller's copy of the B*N*3 integers is the only one."""
    lib = _lib.load()
    if not (pts.is_cuda and offs.is_cuda):
        raise _lib.PrgError("expected tensors on the HIP device (this package has no CPU path)")
    assert pts.dtype == torch.float32 and offs.dtype == torch.int64
    dev = pts.device
    pts, offs = pts.contiguous().view(-1, 3), offs.contiguous()
    B = offs.numel() - 1
    P = (poses if torch.is_tensor(poses) else torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32))).to(dev, torch.float32)
    Kd = (K if torch.is_tensor(K) else torch.from_numpy(np.ascontiguousarray(K, dtype=np.float32))).to(dev, torch.float32)
    if P.dim() != 4 or P.shape[0] != B or tuple(P.shape[2:]) != (4, 4) or tuple(Kd.shape) != (B, 3, 3):
        raise ValueError("pose_candidate_counts: poses (B,N,4,4) and K (B,3,3) for the B clouds of offs")
    P, Kd = P.contiguous(), Kd.contiguous()
    N = P.shape[1]
    H, W = _image_hw(S)
    b6 = _box6(box)
    counts = torch.empty((B, N, 3), dtype=torch.int32, device=dev)
    nbytes = int(lib.prg_pose_candidate_workspace_bytes(B, N, H, W)) if workspace_bytes is None else int(workspace_bytes)
    ws = _voxel_workspace(dev, nbytes) if workspace_bytes is None else torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
    _lib.check(lib.prg_pose_candidate_counts(_lib.ptr(pts), _lib.ptr(offs), _lib.ptr(P), _lib.ptr(Kd), B, N, H, W,
                                             None if b6 is None else b6.ctypes.data, float(z_tol), _lib.ptr(counts), _lib.ptr(ws),
                                             nbytes, _lib.stream_ptr()), "prg_pose_candidate_counts")
    return counts


def unproject_f64(depth: torch.Tensor, intrinsic: torch.Tensor, pose: Optional[torch.Tensor], *,
                  depth_unit: float = DEPTH_UNIT_M, clip=(0.5, 10.0)):
    """Batched float64 `point_cloud` + inverse pose (sd:122-143, sd:2623-2628) -> xyz (B,HW,3) f64, valid (B,HW)."""
    lib = _lib.load()
    depth, K = _f32(depth), _f32(intrinsic)
    P = None if pose is None else _f32(pose)
    B, Cc, H, W = depth.shape
    xyz = torch.empty((B, H * W, 3), dtype=torch.float64, device=depth.device)
    valid = torch.empty((B, H * W), dtype=torch.uint8, device=depth.device)
    _lib.check(lib.prg_unproject_f64(_lib.ptr(depth), _lib.ptr(K), _lib.ptr(P), _lib.ptr(xyz), _lib.ptr(valid), B, H, W,
                                     float(depth_unit), float(clip[0]), float(clip[1]), _lib.stream_ptr()),
               "prg_unproject_f64")
    return xyz, valid.view(torch.bool)


_VOXEL_WORKSPACE = {}     # (device index, stream) -> uint8 tensor: lanes of one device run on their own streams


def _voxel_workspace(device, nbytes: int) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    ws = _VOXEL_WORKSPACE.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=device)
        _VOXEL_WORKSPACE[key] = ws
    return ws


def voxel_grid_ragged(pts: torch.Tensor, valid: Optional[torch.Tensor], offsets: torch.Tensor, voxel: float):
    """PointCloud.voxel_down_sample of B ragged clouds in one call, on the device (prg_voxel_grid_ragged): pts (total,3)
    float64, valid (total) bool / uint8 or None, offsets (B+1) int64, all device tensors.  Returns (out (total,3) float64,
    out_offsets (B+1) int64, status (B) int32) on the device: segment b's voxel means are out[out_offsets[b]:out_offsets[b+1]],
    bit for bit what `postprocess.native_voxel_down_sample` returns for its valid rows; status 1 = non-finite row,
    2 = grid too large (such a segment has no rows).  Nothing is copied to the host and nothing synchronises."""
    lib = _lib.load()
    pts, offsets, total = _ragged_f64(pts, offsets)
    B = offsets.numel() - 1
    v8 = _u8(valid)
    assert v8 is None or v8.numel() == total
    out = torch.empty((max(total, 1), 3), dtype=torch.float64, device=pts.device)
    out_offsets = torch.empty((B + 1,), dtype=torch.int64, device=pts.device)
    status = torch.empty((B,), dtype=torch.int32, device=pts.device)
    nbytes = int(lib.prg_voxel_grid_workspace_bytes(total, B))
    ws = _voxel_workspace(pts.device, nbytes)
    _lib.check(lib.prg_voxel_grid_ragged(_lib.ptr(pts), _lib.ptr(v8), _lib.ptr(offsets), B, total, float(voxel),
                                         _lib.ptr(out), _lib.ptr(out_offsets), _lib.ptr(status), _lib.ptr(ws), ws.numel(),
                                         _lib.stream_ptr()), "prg_voxel_grid_ragged")
    return out[:total], out_offsets, status


def overlap_counts_indexed(pts: torch.Tensor, offsets: torch.Tensor, pair_index: torch.Tensor, max_cloud: int, radius: float):
    """prg_overlap_counts_indexed: pts (total,3) float64 and offsets (n_clouds+1) int64, a SET of ragged clouds, and pair_index
    (n_pairs,2) int32, all device tensors.  -> counts (n_pairs,2) int32 on the device: for (s, t) = pair_index[p] the rows of
    cloud s with a row of cloud t strictly within `radius`, and the same from t's side — `prg_overlap_counts`' decision, every
    cloud stored once however many pairs it is in.  A pair with an entry outside [0, n_clouds) gets (-1, -1).  At most 65535
    pairs per call.  Nothing synchronises."""
    lib = _lib.load()
    pts, offsets, _total = _ragged_f64(pts, offsets)
    if not pair_index.is_cuda:
        raise _lib.PrgError("expected tensors on the HIP device (this package has no CPU path)")
    assert pair_index.dtype == torch.int32 and pair_index.dim() == 2 and pair_index.shape[1] == 2
    pair_index = pair_index.contiguous()
    n_pairs = pair_index.shape[0]
    counts = torch.empty((n_pairs, 2), dtype=torch.int32, device=pts.device)
    _lib.check(lib.prg_overlap_counts_indexed(_lib.ptr(pts), _lib.ptr(offsets), offsets.numel() - 1, _lib.ptr(pair_index), n_pairs,
                                              int(max_cloud), float(radius), _lib.ptr(counts), _lib.stream_ptr()),
               "prg_overlap_counts_indexed")
    return counts


def nearest_ragged(pts: torch.Tensor, offsets: torch.Tensor, n_pairs: int, max_cloud: int):
    """Nearest point of the other cloud for `n_pairs` cloud pairs in one launch (prg_nearest_ragged_f64): pts (total,3)
    float64 and offsets (2*n_pairs+1) int64 as `prg_overlap_counts` takes them, both device tensors.  Returns (d2 (total)
    float64, idx (total) int32) on the device: per row the smallest squared distance to a row of its pair's other cloud and
    the lowest local row that attains it, bit for bit `postprocess.nearest`; +inf / -1 where there is none.  Entries of rows
    outside every segment are +inf / -1 as allocated here (the kernel does not touch them).  Nothing synchronises."""
    lib = _lib.load()
    pts, offsets, total = _ragged_f64(pts, offsets, n_pairs)
    d2 = torch.full((total,), float("inf"), dtype=torch.float64, device=pts.device)
    idx = torch.full((total,), -1, dtype=torch.int32, device=pts.device)
    _lib.check(lib.prg_nearest_ragged_f64(_lib.ptr(pts), _lib.ptr(offsets), int(n_pairs), int(max_cloud), _lib.ptr(d2),
                                          _lib.ptr(idx), _lib.stream_ptr()), "prg_nearest_ragged_f64")
    return d2, idx


def radius_pairs_ragged(pts: torch.Tensor, offsets: torch.Tensor, n_pairs: int, max_cloud: int, radius: float):
    """All pairs within `radius` for `n_pairs` cloud pairs (prg_radius_count_ragged_f64 / prg_radius_fill_ragged_f64): pts
    (total,3) float64 and offsets (2*n_pairs+1) int64 as `prg_overlap_counts` takes them, both device tensors; pair p queries
    segment 2p against segment 2p+1.  Returns (corr (K,2) int32, pair_offsets (n_pairs+1) int64) on the device: pair p's
    correspondences are corr[pair_offsets[p]:pair_offsets[p+1]], rows (i, j) local to the two clouds, ordered by i then j, bit for
    bit `postprocess.radius_pairs`.  Count, ONE 8-byte read-back (the size of the list — the only synchronisation), an
    allocation of exactly K rows, fill."""
    pts, offsets, total = _ragged_f64(pts, offsets, n_pairs)
    row_start, corr, _ = _count_fill(pts, offsets, int(n_pairs), total, max_cloud, radius)
    return corr, row_start[offsets[0::2]]


def _count_fill(pts, offsets, n_pairs: int, total: int, max_cloud, radius, also: Optional[torch.Tensor] = None):
    """prg_radius_count_ragged_f64, the read-back of the list size K — THE synchronisation: 8 bytes, or 16 in one copy with
    `also`, a device int64 scalar the caller wants on the host as well —, an allocation of exactly K rows, and
    prg_radius_fill_ragged_f64 unless K == 0.  -> (row_start (total+1) int64, corr (K,2) int32, `also` as an int or None)."""
    lib = _lib.load()
    dev = pts.device
    row_start = torch.empty((total + 1,), dtype=torch.int64, device=dev)
    ws = _voxel_workspace(dev, int(lib.prg_radius_pairs_workspace_bytes(total)))
    _lib.check(lib.prg_radius_count_ragged_f64(_lib.ptr(pts), _lib.ptr(offsets), n_pairs, total, int(max_cloud), float(radius),
                                               _lib.ptr(row_start), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "prg_radius_count_ragged_f64")
    if also is None:
        K = int(row_start[total].item())
    else:
        K, also = (int(v) for v in torch.stack([row_start[total], also]).tolist())
    corr = torch.empty((K, 2), dtype=torch.int32, device=dev)
    if K:
        _lib.check(lib.prg_radius_fill_ragged_f64(_lib.ptr(pts), _lib.ptr(offsets), n_pairs, int(max_cloud), float(radius),
                                                  _lib.ptr(row_start), K, _lib.ptr(corr), _lib.stream_ptr()),
                   "prg_radius_fill_ragged_f64")
    return row_start, corr, also


def _neighbor_tables(pts, offsets, n_pairs, max_cloud, radius, limit, index_base, pad, query_rows=None):
    """count / fill / select on one pair buffer -> (table, table_offsets, count).  `query_rows`: the total number of query rows
    when the caller already has it on the host; then the read-back is the 8 bytes of the list size alone."""
    lib = _lib.load()
    pts, offsets, total = _ragged_f64(pts, offsets, n_pairs)
    n_pairs, limit, total = int(n_pairs), int(limit), max(total, 1)     # the stand-in row of an empty buffer counts as a row
    if not 1 <= limit <= 1024:
        raise _lib.PrgError("radius_neighbors_ragged: limit must be in 1..1024")
    dev = pts.device
    for t in (index_base, pad):
        assert t is None or (t.is_cuda and t.dtype == torch.int32 and t.numel() == n_pairs)
    table_offsets = torch.zeros((n_pairs + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(offsets[1::2] - offsets[0:-1:2], 0, out=table_offsets[1:])
    row_start, corr, Q = _count_fill(pts, offsets, n_pairs, total, max_cloud, radius,
                                     also=table_offsets[n_pairs] if query_rows is None else None)
    K, Q = corr.shape[0], int(query_rows if query_rows is not None else Q)
    table = torch.empty((Q, limit), dtype=torch.int32, device=dev)
    count = torch.empty((Q,), dtype=torch.int32, device=dev)
    if Q == 0:
        return table, table_offsets, count
    _lib.check(lib.prg_radius_select_ragged_f64(_lib.ptr(pts), _lib.ptr(offsets), n_pairs, int(max_cloud), _lib.ptr(row_start),
                                                _lib.ptr(corr), K, limit, _lib.ptr(table_offsets),
                                                _lib.ptr(None if index_base is None else index_base.contiguous()),
                                                _lib.ptr(None if pad is None else pad.contiguous()), _lib.ptr(table),
                                                _lib.stream_ptr()), "prg_radius_select_ragged_f64")
    # count = row_start differences over the query rows: table row t belongs to pair p = the last p with table_offsets[p] <= t
    t = torch.arange(Q, dtype=torch.int64, device=dev)
    p = torch.searchsorted(table_offsets[1:].contiguous(), t, right=True)
    q = offsets[0::2][p] + (t - table_offsets[p])
    torch.sub(row_start[q + 1], row_start[q], out=count)
    return table, table_offsets, count


def radius_neighbors_ragged(pts: torch.Tensor, offsets: torch.Tensor, n_pairs: int, max_cloud: int, radius: float, limit: int,
                            index_base: Optional[torch.Tensor] = None, pad: Optional[torch.Tensor] = None):
    """Neighbour tables for `n_pairs` cloud pairs: per query row its `limit` nearest candidates within `radius`, nearest first
    (prg_radius_count_ragged_f64 / prg_radius_fill_ragged_f64, then prg_radius_select_ragged_f64).  pts (total,3) float64 and
    offsets (2*n_pairs+1) int64 as `radius_pairs_ragged` takes them, both device tensors; pair p queries segment 2p against
    segment 2p+1.  index_base / pad: (n_pairs) int32 device tensors or None — a match j of pair p is written as index_base[p] + j
    (None: j), an empty slot as pad[p] (None: the rows of the candidate cloud).
    Returns (table (Q, limit) int32, table_offsets (n_pairs+1) int64, count (Q) int32) on the device, Q = all query rows: pair p's
    table is table[table_offsets[p]:table_offsets[p+1]], bit for bit `postprocess.radius_neighbors` of its two clouds, and count
    the matches per row before truncation (row_start differences).  Count, ONE read-back (the size of the list and Q, 16 bytes in
    one copy — the only synchronisation), allocations of exactly K and Q rows, fill, select."""
    return _neighbor_tables(pts, offsets, n_pairs, max_cloud, radius, limit, index_base, pad)


def neighbor_pyramid(points: torch.Tensor, lengths, *, num_stages: int, voxel_size: float, radius: float, neighbor_limits):
    """The KPConv pyramid of a stack of C clouds on the device, bit for bit `postprocess.neighbor_pyramid` (which states the
    definition): points (N,3) float64 or float32 device tensor — float32 is widened, which is exact — the clouds one after the
    other, lengths (C,) their rows (device tensor, numpy or a list).  Returns {"points", "lengths", "neighbors", "subsampling",
    "upsampling": lists of device tensors per level, "counts": {"neighbors", "subsampling", "upsampling"}}: points float64,
    lengths int64, tables int32 indices into the candidate level's stack with that level's row count as the pad.

    Level l+1 is `voxel_grid_ragged` of level l at voxel_size * 2**(l+1); a non-zero status raises through `check_voxel_status`.
    Two select launches per level: neighbors[l] and subsampling[l] share the radius r_l and the candidates, so they are the 2C
    pairs of ONE count / fill / select; upsampling[l] (radius 2 r_l) is a second one of C pairs; the last level has neighbors only.
    A pair's query and candidate segments are adjacent in the pair buffer, so a level searched against itself needs every cloud
    twice: the buffer [c, c for every cloud, then next-level c, c for every cloud] is assembled by ONE device `cat` of row
    slices per launch — no kernel of its own, 3 N_l + N_{l+1} rows for the first launch, N_l + N_{l+1} for the second.
    Host synchronisations: one for `lengths` if it is a device tensor; then per level l < num_stages - 1 three — one read of
    the next level's offsets and status (C+1 and C numbers in one copy, needed for the slices) and the 8-byte list size of each
    of the two launches; the last level has one (its list size)."""
    if not points.is_cuda:
        raise _lib.PrgError("expected a tensor on the HIP device (this package has no CPU path)")
    if points.dtype not in (torch.float64, torch.float32):
        raise _lib.PrgError("neighbor_pyramid: points must be float64 or float32")
    num_stages = int(num_stages)
    limits = [int(k) for k in neighbor_limits]
    if num_stages < 1 or len(limits) != num_stages:
        raise ValueError("num_stages >= 1 and one neighbor limit per stage")
    if not (np.isfinite(radius) and radius > 0 and np.isfinite(voxel_size) and voxel_size > 0):
        raise ValueError("radius and voxel_size must be finite and > 0")
    dev = points.device
    pts = points.contiguous().view(-1, 3).to(torch.float64)
    lens = (lengths.cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)).astype(np.int64).reshape(-1)
    C = len(lens)
    if C < 1 or (lens < 0).any() or int(lens.sum()) != pts.shape[0]:
        raise ValueError("lengths do not add up to the rows of points")
    max_cloud = max(1, int(lens.max()))             # a level never has more rows per cloud than the one above it

    def launch(segs, n_pairs, r, limit, base, pad):
        """segs: [(level points, start, stop), ...], 2 per pair -> the tables of the launch."""
        sizes = np.array([b - a for _, a, b in segs], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        rows = [P[a:b] for P, a, b in segs if b > a]
        buf = torch.cat(rows, 0) if rows else torch.zeros((1, 3), dtype=torch.float64, device=dev)
        table, _, count = _neighbor_tables(buf, _dev_i64(offs, dev), n_pairs, max_cloud, r, limit, _dev_i32(base, dev),
                                           _dev_i32(pad, dev), query_rows=int(sizes[0::2].sum()))
        return table, count

    out = {"points": [pts], "lengths": [_dev_i64(lens, dev)], "neighbors": [], "subsampling": [], "upsampling": [],
           "counts": {"neighbors": [], "subsampling": [], "upsampling": []}}
    P, o = pts, np.concatenate([[0], np.cumsum(lens)])                  # this level: points, host offsets
    for l in range(num_stages):
        r, N = float(radius) * 2 ** l, int(o[-1])
        segs = [(P, o[c], o[c + 1]) for c in range(C) for _ in range(2)]
        base, pad = list(o[:C]), [N] * C
        if l == num_stages - 1:
            table, count = launch(segs, C, r, limits[l], base, pad)
            out["neighbors"].append(table)
            out["counts"]["neighbors"].append(count)
            break
        if N:
            down, d_offs, status = voxel_grid_ragged(P, None, _dev_i64(o, dev), float(voxel_size) * 2 ** (l + 1))
            host = torch.cat([d_offs, status.to(torch.int64)]).cpu().numpy()
            on = host[:C + 1]
            check_voxel_status(host[C + 1:], ["cloud {} of level {}".format(c, l) for c in range(C)])
        else:                                       # a stack without rows stays one
            down, on = P, o
        Pn, Nn = down[:int(on[-1])], int(on[-1])
        segs += [(Pk, ok[c], ok[c + 1]) for c in range(C) for Pk, ok in ((Pn, on), (P, o))]
        table, count = launch(segs, 2 * C, r, limits[l], base + base, pad + pad)
        out["neighbors"].append(table[:N])
        out["subsampling"].append(table[N:])
        out["counts"]["neighbors"].append(count[:N])
        out["counts"]["subsampling"].append(count[N:])
        segs = [(Pk, ok[c], ok[c + 1]) for c in range(C) for Pk, ok in ((P, o), (Pn, on))]
        table, count = launch(segs, C, 2 * r, limits[l + 1], list(on[:C]), [Nn] * C)
        out["upsampling"].append(table)
        out["counts"]["upsampling"].append(count)
        out["points"].append(Pn)
        out["lengths"].append(_dev_i64(np.diff(on), dev))
        P, o = Pn, on
    return out


def normals_from_tables(points: torch.Tensor, lengths, table: torch.Tensor, count: torch.Tensor, *, viewpoints=None,
                        min_neighbors: int = 3, want_variation: bool = False):
    """Oriented normals of a stack of C clouds from neighbour tables the caller already holds — `neighbor_pyramid(...)
    ["neighbors"][0]` and `["counts"]["neighbors"][0]`, or `estimate_normals`' own search: ONE launch of prg_normals_ragged_f64,
    bit for bit `postprocess.estimate_normals` per cloud (which states the definition).  points (N,3) float64 or float32 device
    tensor (float32 is widened, which is exact), the clouds one after the other; lengths (C,) their rows (device tensor, numpy or
    a list); table (N, limit) int32 with indices into the stack, row t for row t of points; count (N,) int32, the matches before
    truncation.  viewpoints: (C,3), host or device, or None for the origin; every cloud's normals face its own.
    Returns normals (N,3) float64 on the device; with want_variation (normals, variation (N,)).  No host synchronisation: a
    device `lengths` is summed on the device."""
    lib = _lib.load()
    if not (points.is_cuda and table.is_cuda and count.is_cuda):
        raise _lib.PrgError("expected tensors on the HIP device (this package has no CPU path)")
    if points.dtype not in (torch.float64, torch.float32):
        raise _lib.PrgError("normals_from_tables: points must be float64 or float32")
    if int(min_neighbors) != min_neighbors or min_neighbors < 3:
        raise ValueError("min_neighbors must be an integer >= 3")
    dev = points.device
    pts = points.contiguous().view(-1, 3).to(torch.float64)
    N = pts.shape[0]
    lens = lengths.to(torch.int64).view(-1) if torch.is_tensor(lengths) else _dev_i64(np.asarray(lengths).reshape(-1), dev)
    C = lens.numel()
    if table.dtype != torch.int32 or count.dtype != torch.int32 or table.dim() != 2 or table.shape[0] != N or count.numel() != N:
        raise ValueError("table must be (rows of points, limit) int32 and count (rows of points,) int32")
    if not 1 <= C <= 65535:
        raise ValueError("1..65535 clouds")
    if viewpoints is None:
        views = torch.zeros((C, 3), dtype=torch.float64, device=dev)
    elif torch.is_tensor(viewpoints):
        views = viewpoints.to(device=dev, dtype=torch.float64).contiguous().view(-1, 3)
    else:
        views = torch.from_numpy(np.ascontiguousarray(viewpoints, dtype=np.float64).reshape(-1, 3)).to(dev)
    if views.shape[0] != C:
        raise ValueError("one viewpoint per cloud")
    offsets = torch.zeros((C + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=offsets[1:])
    normals = torch.empty((N, 3), dtype=torch.float64, device=dev)
    variation = torch.empty((N,), dtype=torch.float64, device=dev) if want_variation else None
    if N:
        _lib.check(lib.prg_normals_ragged_f64(_lib.ptr(pts), _lib.ptr(offsets), C, _lib.ptr(table.contiguous()), _lib.ptr(offsets),
                                              None, _lib.ptr(count.contiguous()), N, int(table.shape[1]), _lib.ptr(views),
                                              int(min_neighbors), _lib.ptr(normals), _lib.ptr(variation), None,
                                              _lib.stream_ptr()), "prg_normals_ragged_f64")
    return (normals, variation) if want_variation else normals


def estimate_normals(points: torch.Tensor, lengths, *, radius: float = 0.1, limit: int = 30, viewpoints=None,
                     min_neighbors: int = 3, want_variation: bool = False):
    """Oriented surface normals of a stack of C clouds on the device, bit for bit `postprocess.estimate_normals_cloud(cloud_c,
    radius, limit, viewpoints[c])` per cloud: per row the PCA normal of its `limit` nearest rows within `radius` (itself
    included; open3d's KDTreeSearchParamHybrid(radius, max_nn=limit)), turned towards its cloud's viewpoint.  points (N,3)
    float64 or float32 device tensor, the clouds one after the other; lengths (C,) their rows (device tensor, numpy or a list);
    viewpoints (C,3), host or device, or None: the origin for every cloud.  Returns normals (N,3) float64 on the device, and
    (normals, variation (N,)) with want_variation.  A host tensor raises PrgError: there is no CPU path.

    The pair buffer [c, c for every cloud] of a self-search is assembled as `neighbor_pyramid` does for one level (ONE device
    `cat` of row slices, 2 N rows), then ONE count / fill / select (`_neighbor_tables`) and ONE launch of the normals kernel
    (`normals_from_tables`).  Host synchronisations: one for `lengths` if it is a device tensor (the slices need it), and the
    8-byte list size of the search; the normals kernel adds none."""
    if not points.is_cuda:
        raise _lib.PrgError("expected a tensor on the HIP device (this package has no CPU path)")
    if points.dtype not in (torch.float64, torch.float32):
        raise _lib.PrgError("estimate_normals: points must be float64 or float32")
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be finite and > 0")
    if int(limit) != limit or not 1 <= limit <= 1024:
        raise ValueError("limit must be an integer in 1..1024")
    dev = points.device
    pts = points.contiguous().view(-1, 3).to(torch.float64)
    lens = (lengths.cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)).astype(np.int64).reshape(-1)
    C, N = len(lens), pts.shape[0]
    if C < 1 or (lens < 0).any() or int(lens.sum()) != N:
        raise ValueError("lengths do not add up to the rows of points")
    o = np.concatenate([[0], np.cumsum(lens)])
    if N:
        buf = torch.cat([pts[o[c]:o[c + 1]] for c in range(C) for _ in range(2) if lens[c]], 0)
        offs = np.concatenate([[0], np.cumsum(np.repeat(lens, 2))])
        table, _, count = _neighbor_tables(buf, _dev_i64(offs, dev), C, int(lens.max()), float(radius), int(limit),
                                           _dev_i32(o[:C], dev), _dev_i32([N] * C, dev), query_rows=N)
    else:
        table = torch.empty((0, int(limit)), dtype=torch.int32, device=dev)
        count = torch.empty((0,), dtype=torch.int32, device=dev)
    return normals_from_tables(pts, lens, table, count, viewpoints=viewpoints, min_neighbors=min_neighbors,
                               want_variation=want_variation)


def _host_offsets(o, what: str) -> np.ndarray:
    """CSR offsets as a host int64 array; a device tensor is copied back (one synchronisation)."""
    o = (o.cpu().numpy() if torch.is_tensor(o) else np.asarray(o)).astype(np.int64).reshape(-1)
    if len(o) < 2 or (np.diff(o) < 0).any() or o[0] < 0:
        raise ValueError("{}: ascending offsets with at least two entries".format(what))
    return o


def _check_patch_limit(limit, what: str) -> int:
    if int(limit) != limit or not 1 <= limit <= 256:
        raise _lib.PrgError("{}: limit must be in 1..256".format(what))
    return int(limit)


def node_patches_ragged(points: torch.Tensor, point_offsets, nodes: torch.Tensor, node_offsets, limit: int,
                        index_base: Optional[torch.Tensor] = None, pad: Optional[torch.Tensor] = None):
    """The point-to-node partition of C clouds and its per-node tables, bit for bit `postprocess.node_patches` per cloud: points
    (N,3) and nodes (M,3) float64 device tensors, point_offsets / node_offsets (C+1) CSR offsets (numpy, a list or tensors); cloud
    c's points are points[point_offsets[c]:point_offsets[c+1]], its nodes likewise.  index_base / pad: (C) int32 device tensors or
    None — a member i of cloud c is written as index_base[c] + i (None: i, the row counted from the cloud's first point), an empty
    slot as pad[c] (None: the rows of the cloud).
    Returns (assign (N) int32 — per point its node counted from the cloud's first node, -1 for none and for rows outside every
    cloud; table (rows, limit) int32 and sizes (rows) int32, rows = node_offsets[C] - node_offsets[0]: node k of cloud c is row
    node_offsets[c] - node_offsets[0] + k) on the device.
    One device `cat` of row slices into the pair layout [points_c | nodes_c], `nearest_ragged` on it (prg_nearest_ragged_f64),
    a gather of the point rows' assignment, prg_patch_tables_ragged.  Host synchronisations: none when both offsets are on the
    host; one copy back per offsets tensor that is on the device."""
    lib = _lib.load()
    if not (points.is_cuda and nodes.is_cuda):
        raise _lib.PrgError("expected tensors on the HIP device (this package has no CPU path)")
    assert points.dtype == torch.float64 and nodes.dtype == torch.float64
    limit = _check_patch_limit(limit, "node_patches_ragged")
    dev = points.device
    points, nodes = points.contiguous().view(-1, 3), nodes.contiguous().view(-1, 3)
    po, no = _host_offsets(point_offsets, "point_offsets"), _host_offsets(node_offsets, "node_offsets")
    C = len(po) - 1
    if len(no) != C + 1 or po[-1] > points.shape[0] or no[-1] > nodes.shape[0]:
        raise ValueError("offsets do not fit the clouds")
    for t in (index_base, pad):
        assert t is None or (t.is_cuda and t.dtype == torch.int32 and t.numel() == C)
    rows = int(no[-1] - no[0])
    assign = torch.full((points.shape[0],), -1, dtype=torch.int32, device=dev)
    table = torch.empty((rows, limit), dtype=torch.int32, device=dev)
    sizes = torch.empty((rows,), dtype=torch.int32, device=dev)
    if rows == 0:                                   # no node anywhere: nothing to write, every point stays at -1
        return assign, table, sizes
    seg = np.stack([np.diff(po), np.diff(no)], 1).reshape(-1)                       # rows of [points_0, nodes_0, points_1, ...]
    offs = np.concatenate([[0], np.cumsum(seg)]).astype(np.int64)
    parts = [t[int(o[c]):int(o[c + 1])] for c in range(C) for t, o in ((points, po), (nodes, no)) if o[c + 1] > o[c]]
    buf = torch.cat(parts, 0)
    d_offs = torch.from_numpy(offs).to(dev)
    max_cloud, max_nodes = max(1, int(seg[0::2].max())), max(1, int(seg[1::2].max()))
    d2, idx = nearest_ragged(buf, d_offs, C, max(max_cloud, max_nodes))
    t_offs = torch.from_numpy(np.ascontiguousarray(no[:-1] - no[0])).to(dev)
    base = None if index_base is None else index_base.contiguous()      # named: a temporary's block could be handed out again
    padv = None if pad is None else pad.contiguous()                    # before the launch
    _lib.check(lib.prg_patch_tables_ragged(_lib.ptr(d2), _lib.ptr(idx), _lib.ptr(d_offs), C, max_cloud, max_nodes, limit,
                                           _lib.ptr(t_offs), _lib.ptr(base), _lib.ptr(padv), _lib.ptr(table), _lib.ptr(sizes),
                                           _lib.stream_ptr()), "prg_patch_tables_ragged")
    if po[-1] > po[0]:
        assign[int(po[0]):int(po[-1])] = torch.cat([idx[int(offs[2 * c]):int(offs[2 * c + 1])] for c in range(C) if seg[2 * c]], 0)
    return assign, table, sizes


def patch_overlaps_ragged(pts: torch.Tensor, offsets, tables: torch.Tensor, table_offsets, radius: float, *,
                          prefilter: bool = True):
    """Which node patches overlap, for n items at once, bit for bit `postprocess.patch_overlaps` per item: pts (total,3) float64
    device tensor and offsets (2n+1) as `prg_overlap_counts` takes them — segment 2p the fine points of item p's source cloud,
    segment 2p+1 of its target; tables (rows, limit) int32 device tensor, the patch tables of all 2n clouds with LOCAL point rows
    and the cloud's row count as the pad (`node_patches_ragged` with index_base = pad = None), table_offsets (2n+1) the first
    table row of every cloud and the end.  Both offsets: numpy, a list or tensors.
    Returns (node_corr (P,2) int32 — (source node, target node) counted from each cloud's first node, ordered by item, a, b;
    hits (P,2) int32; overlap (P,) float64; corr_offsets (n+1) int64: item p's rows are [corr_offsets[p], corr_offsets[p+1])) on
    the device.  prg_patch_overlap_ragged_f64 writes the two hit counts of EVERY node pair (dense, 8 bytes per pair, at most 2^28
    pairs per call); `nonzero` over them, a gather and the float64 overlap in torch follow.  prefilter: the kernel's exact
    bounding-box test (False runs every patch pair; the result is the same).
    Host synchronisations: ONE, the number of listed node pairs inside `nonzero`; one more per offsets tensor that is on the
    device."""
    lib = _lib.load()
    if not (pts.is_cuda and tables.is_cuda):
        raise _lib.PrgError("expected tensors on the HIP device (this package has no CPU path)")
    assert pts.dtype == torch.float64 and tables.dtype == torch.int32 and tables.dim() == 2
    if not (np.isfinite(radius) and radius > 0):
        raise _lib.PrgError("patch_overlaps_ragged: radius must be finite and > 0")
    dev = pts.device
    pts, tables = pts.contiguous().view(-1, 3), tables.contiguous()
    limit = _check_patch_limit(tables.shape[1], "patch_overlaps_ragged")
    o, to = _host_offsets(offsets, "offsets"), _host_offsets(table_offsets, "table_offsets")
    n = (len(o) - 1) // 2
    if len(o) != 2 * n + 1 or n < 1 or len(to) != len(o) or o[-1] > pts.shape[0] or to[-1] > tables.shape[0]:
        raise ValueError("offsets do not fit the clouds or the tables")
    m = np.diff(to)
    per_item = m[0::2] * m[1::2]
    ho = np.concatenate([[0], np.cumsum(per_item)]).astype(np.int64)
    total = int(ho[-1])
    if total > 1 << 28:
        raise _lib.PrgError("patch_overlaps_ragged: more than 2^28 node pairs in one call")
    hits = torch.empty((total, 2), dtype=torch.int32, device=dev)
    d_o, d_to, d_ho, d_m = (_dev_i64(a, dev) for a in (o, to, ho, m))   # named: a temporary's block could be handed out again
    if total:
        if pts.shape[0] == 0:                       # no rows: a tensor without elements has no address to pass
            pts = torch.zeros((1, 3), dtype=torch.float64, device=dev)
        boxes = torch.empty((tables.shape[0], 6), dtype=torch.float64, device=dev) if prefilter else None
        _lib.check(lib.prg_patch_overlap_ragged_f64(_lib.ptr(pts), _lib.ptr(d_o), n, _lib.ptr(tables), _lib.ptr(d_to),
                                                    int(m.max()), limit, float(radius), _lib.ptr(d_ho), total,
                                                    int(per_item.max()), _lib.ptr(boxes), _lib.ptr(hits), _lib.stream_ptr()),
                   "prg_patch_overlap_ragged_f64")
    g = torch.nonzero(hits[:, 0] > 0).view(-1)                                    # THE synchronisation; ascending = (item, a, b)
    p = torch.searchsorted(d_ho[1:].contiguous(), g, right=True)                  # the item of every listed node pair
    local = g - d_ho[p]
    mt = d_m[2 * p + 1]
    a, b = torch.div(local, mt, rounding_mode="floor"), torch.remainder(local, mt)
    listed = hits[g]
    # |patch| = the entries of a table row that are not the pad, i.e. not the row count of the row's cloud
    rows_of = torch.repeat_interleave(_dev_i64(np.diff(o), dev), d_m, output_size=int(to[-1] - to[0]))
    size = (tables[int(to[0]):int(to[-1])] != rows_of[:, None].to(torch.int32)).sum(1).to(torch.float64)
    size_a, size_b = size[d_to[2 * p] - int(to[0]) + a], size[d_to[2 * p + 1] - int(to[0]) + b]
    overlap = (listed[:, 0].to(torch.float64) / size_a + listed[:, 1].to(torch.float64) / size_b) / 2
    corr_offsets = torch.searchsorted(g, d_ho)
    return torch.stack([a, b], 1).to(torch.int32), listed, overlap, corr_offsets


def coarse_ground_truth(pyr: dict, *, fine_level: int, limit: int, radius: float) -> dict:
    """The patch-level ground truth of a coarse-to-fine network on the dict `neighbor_pyramid` returns, bit for bit
    `postprocess.coarse_ground_truth` (which states the definition and the returned keys): the stack is [src_0, tgt_0, src_1,
    tgt_1, ...], the nodes are the last level, the fine points level `fine_level`.  One `node_patches_ragged` over all clouds
    (local tables), one `patch_overlaps_ragged` over all items, then the stack indices with torch on the device.
    Host synchronisations: one copy back of the two levels' `lengths` (the pyramid keeps them on the device) and the ONE of
    `patch_overlaps_ragged`."""
    limit = _check_patch_limit(limit, "coarse_ground_truth")
    levels = len(pyr["points"])
    if int(fine_level) != fine_level or not 0 <= fine_level < levels:
        raise ValueError("fine_level must be in 0..num_stages-1")
    fine, nodes = pyr["points"][int(fine_level)], pyr["points"][-1]
    if not (fine.is_cuda and nodes.is_cuda):
        raise _lib.PrgError("expected a pyramid on the HIP device (this package has no CPU path)")
    dev = fine.device
    lens = torch.stack([pyr["lengths"][int(fine_level)].to(torch.int64), pyr["lengths"][-1].to(torch.int64)]).cpu().numpy()
    fl, nl = lens[0], lens[1]
    if len(fl) % 2 or len(fl) < 2:
        raise ValueError("the stack must hold an even number of clouds: [src_0, tgt_0, src_1, tgt_1, ...]")
    fo, no = np.concatenate([[0], np.cumsum(fl)]), np.concatenate([[0], np.cumsum(nl)])
    assign, local, sizes = node_patches_ragged(fine, fo, nodes, no, limit)
    corr, hits, overlap, corr_offsets = patch_overlaps_ragged(fine, fo, local, no, radius)
    # local rows -> rows of the level's stack, as the pyramid's tables are indexed
    node_base = torch.repeat_interleave(_dev_i32(no[:-1], dev), torch.from_numpy(fl).to(dev), output_size=int(fo[-1]))
    point_base = torch.repeat_interleave(_dev_i32(fo[:-1], dev), torch.from_numpy(nl).to(dev), output_size=int(no[-1]))
    rows_of = torch.repeat_interleave(_dev_i32(fl, dev), torch.from_numpy(nl).to(dev), output_size=int(no[-1]))
    assign = torch.where(assign >= 0, assign + node_base, assign)
    table = torch.where(local != rows_of[:, None], local + point_base[:, None], torch.full_like(local, int(fo[-1])))
    item = torch.searchsorted(corr_offsets[1:].contiguous(), torch.arange(corr.shape[0], device=dev), right=True)
    d_no = _dev_i32(no, dev)
    node_corr = corr + torch.stack([d_no[2 * item], d_no[2 * item + 1]], 1)
    return {"assign": assign, "table": table, "sizes": sizes, "node_corr": node_corr, "hits": hits, "overlap": overlap,
            "corr_offsets": corr_offsets}


def patch_corr_labels(points: torch.Tensor, table: torch.Tensor, pairs: torch.Tensor, radius: float) -> torch.Tensor:
    """The fine-level label matrices of S selected patch pairs, bit for bit `postprocess.patch_corr_labels` (which states the
    definition): points (N,3) float64 device tensor (float32 is converted), the fine level's stack; table (M,K) int32 device
    tensor, the patches as rows of that stack, an entry outside [0, N) a pad (`coarse_ground_truth`'s "table"); pairs (S,2) int32
    device tensor, rows of `table` as (source node, target node).  Returns (S, K+1, K+1) torch.bool on the device, a view of the
    uint8 buffer prg_patch_corr_labels_f64 wrote (one launch per 2^24 pairs).  S == 0 returns the empty tensor without a launch.
    Host synchronisations: none."""
    lib = _lib.load()
    if not (points.is_cuda and table.is_cuda and pairs.is_cuda):
        raise _lib.PrgError("expected tensors on the HIP device (this package has no CPU path)")
    if not (np.isfinite(radius) and radius > 0):
        raise _lib.PrgError("patch_corr_labels: radius must be finite and > 0")
    assert table.dtype == torch.int32 and table.dim() == 2 and pairs.dtype == torch.int32
    limit = _check_patch_limit(table.shape[1], "patch_corr_labels")
    points = points.to(torch.float64).contiguous().view(-1, 3)
    table, pairs = table.contiguous(), pairs.contiguous().view(-1, 2)
    N, M, S = points.shape[0], table.shape[0], pairs.shape[0]
    if N >= 1 << 31 or M >= 1 << 31:
        raise _lib.PrgError("patch_corr_labels: 2^31 or more rows")
    if S == 0 or M == 0:                            # no pair, or no node: every pair stands for two empty patches
        return torch.zeros((S, limit + 1, limit + 1), dtype=torch.bool, device=points.device)
    labels = torch.empty((S, limit + 1, limit + 1), dtype=torch.uint8, device=points.device)
    step = 1 << 24
    for s0 in range(0, S, step):
        part, out = pairs[s0:s0 + step], labels[s0:s0 + step]   # named: contiguous views of tensors that outlive the launch
        _lib.check(lib.prg_patch_corr_labels_f64(_lib.ptr(points) if N else None, N, _lib.ptr(table), M, limit, _lib.ptr(part),
                                                 part.shape[0], float(radius), _lib.ptr(out), _lib.stream_ptr()),
                   "prg_patch_corr_labels_f64")
    return labels.view(torch.bool)


def select_node_corr(gt: dict, *, min_overlap: float = 0.1, num_targets: int = 128, keys: Optional[torch.Tensor] = None,
                     generator: Optional[torch.Generator] = None):
    """Which ground-truth node pairs the fine level trains on, bit for bit `postprocess.select_node_corr` on gt["overlap"] and
    gt["corr_offsets"] (`coarse_ground_truth`'s dict, on the device): per item the rows with overlap > min_overlap, and of more
    than `num_targets` of them the `num_targets` with the smallest (keys[r], r).  keys: (P,) float64 device tensor, one per row
    of gt["node_corr"]; None draws torch.rand(P, dtype=float64, generator=generator) on the device — a uniform sample without
    replacement.  Returns (rows (S,) int64 ascending, sel_offsets (items+1,) int64) on the device.  Two stable sorts (by key, then
    by item and candidate flag) rank every candidate within its item; no kernel of this project's.
    Host synchronisations: ONE, the number of selected rows inside `nonzero`."""
    if int(num_targets) != num_targets or num_targets < 1:
        raise ValueError("num_targets must be an integer >= 1")
    overlap, co = gt["overlap"], gt["corr_offsets"]
    if not (overlap.is_cuda and co.is_cuda):
        raise _lib.PrgError("expected a ground truth on the HIP device (this package has no CPU path)")
    dev = overlap.device
    overlap, co = overlap.to(torch.float64).view(-1), co.to(torch.int64).view(-1)
    P = overlap.shape[0]
    if keys is None:
        keys = torch.rand(P, dtype=torch.float64, device=dev, generator=generator)
    keys = keys.to(device=dev, dtype=torch.float64).view(-1)
    if keys.shape[0] != P:
        raise ValueError("one key per listed node pair")
    r = torch.arange(P, device=dev)
    item = torch.searchsorted(co[1:].contiguous(), r, right=True)
    cand = (overlap > min_overlap) & (r >= co[0]) & (r < co[-1])                  # rows outside every item are no candidates
    by_key = torch.sort(keys, stable=True).indices                                # (key, row): rows arrive ascending
    group = 2 * item + (~cand).to(torch.int64)                                    # per item its candidates first
    grouped = torch.sort(group[by_key], stable=True)
    order = by_key[grouped.indices]
    rank = torch.empty_like(r)
    rank[order] = r
    keep = cand & (rank - torch.searchsorted(grouped.values, 2 * item) < int(num_targets))
    rows = torch.nonzero(keep).view(-1)                                           # THE synchronisation; ascending
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(keep.to(torch.int64), 0)])
    return rows, csum[co]


def fine_ground_truth(pyr: dict, gt: dict, *, fine_level: int, radius: float, min_overlap: float = 0.1, num_targets: int = 128,
                      keys: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None) -> dict:
    """The fine-level ground truth of a coarse-to-fine network on the dicts `neighbor_pyramid` and `coarse_ground_truth` return
    (the same `fine_level`), bit for bit `postprocess.fine_ground_truth` (which states the definition and the returned keys):
    `select_node_corr` picks the node pairs, two gathers give their patch tables and masks, ONE prg_patch_corr_labels_f64 writes
    their label matrices.  Everything returned is on the device.
    Host synchronisations: ONE, the number of selected node pairs inside `select_node_corr`."""
    levels = len(pyr["points"])
    if int(fine_level) != fine_level or not 0 <= fine_level < levels:
        raise ValueError("fine_level must be in 0..num_stages-1")
    fine, table = pyr["points"][int(fine_level)], gt["table"]
    if not (fine.is_cuda and table.is_cuda):
        raise _lib.PrgError("expected a pyramid and a ground truth on the HIP device (this package has no CPU path)")
    rows, sel_offsets = select_node_corr(gt, min_overlap=min_overlap, num_targets=num_targets, keys=keys, generator=generator)
    node_corr = gt["node_corr"][rows]
    src_table, tgt_table = table[node_corr[:, 0].to(torch.int64)], table[node_corr[:, 1].to(torch.int64)]
    n_fine = fine.view(-1, 3).shape[0]
    return {"rows": rows, "sel_offsets": sel_offsets, "node_corr": node_corr, "src_table": src_table, "tgt_table": tgt_table,
            "src_mask": src_table != n_fine, "tgt_mask": tgt_table != n_fine,
            "labels": patch_corr_labels(fine, table, node_corr, radius)}


def merge_memory(memory: torch.Tensor, memory_offsets: torch.Tensor, xyz: torch.Tensor, valid: torch.Tensor):
    """Input of a scene-memory update for `voxel_grid_ragged`, without compaction (prg_merge_memory_f64): per scene the
    float32 ragged `memory` rows widened to float64 (valid) followed by the HW rows of xyz[b] with valid[b] as
    `unproject_f64` returns them.  -> (merged (N + B*HW, 3) float64, merged_valid uint8, merged_offsets (B+1) int64)."""
    lib = _lib.load()
    assert memory.is_cuda and memory.dtype == torch.float32 and xyz.dtype == torch.float64
    memory, xyz = memory.contiguous().view(-1, 3), xyz.contiguous()
    B, HW, _ = xyz.shape
    assert memory_offsets.numel() == B + 1 and memory_offsets.dtype == torch.int64
    v8 = _u8(valid)
    rows = memory.shape[0] + B * HW
    merged = torch.empty((rows, 3), dtype=torch.float64, device=xyz.device)
    merged_valid = torch.empty((rows,), dtype=torch.uint8, device=xyz.device)
    merged_offsets = torch.empty((B + 1,), dtype=torch.int64, device=xyz.device)
    _lib.check(lib.prg_merge_memory_f64(_lib.ptr(memory), _lib.ptr(memory_offsets.contiguous()), memory.shape[0],
                                        _lib.ptr(xyz), _lib.ptr(v8), B, HW, _lib.ptr(merged), _lib.ptr(merged_valid),
                                        _lib.ptr(merged_offsets), _lib.stream_ptr()), "prg_merge_memory_f64")
    return merged, merged_valid, merged_offsets


def _transforms(T, B: int, device) -> Optional[torch.Tensor]:
    """(B,4,4) / (B,16) float64, numpy or tensor -> (B,16) float64 on `device` (the 16 doubles are uploaded unchanged)."""
    if T is None:
        return None
    if not torch.is_tensor(T):
        T = torch.from_numpy(np.ascontiguousarray(T, dtype=np.float64))
    assert T.dtype == torch.float64 and T.numel() == 16 * B, "one float64 4x4 per segment"
    return T.to(device).contiguous().view(B, 16)


def _flags(f, B: int, device) -> Optional[torch.Tensor]:
    if f is None:
        return None
    if not torch.is_tensor(f):
        f = torch.from_numpy(np.ascontiguousarray(f).astype(np.uint8))
    assert f.numel() == B
    return _u8(f.to(device))


def rigid_crop_ragged(pts: torch.Tensor, valid: Optional[torch.Tensor], offsets: torch.Tensor, *, T=None, has_T=None,
                      crop=None, out: Optional[torch.Tensor] = None, valid_out: Optional[torch.Tensor] = None):
    """prg_rigid_crop_ragged_f64: segment b of the ragged float64 cloud `pts` (CSR `offsets`, B+1 int64) moved by its row of
    T ((B,4,4) float64; segments with has_T[b] == 0, or all of them when T is None, are copied bit for bit), and, with
    crop = (lo, hi), valid_out = valid && lo <= p' <= hi.  `out` / `valid_out`: where to write (pts / valid themselves for
    in-place use); default: fresh tensors (valid_out only when there is a crop or a mask).  -> (out, valid_out uint8 | None)."""
    lib = _lib.load()
    pts, offsets, total = _ragged_f64(pts, offsets)
    B = offsets.numel() - 1
    v8 = _u8(valid)
    assert v8 is None or v8.numel() == total
    Td, hd = _transforms(T, B, pts.device), _flags(has_T, B, pts.device)
    lo = hi = None
    if crop is not None:
        lo, hi = (np.ascontiguousarray(c, dtype=np.float64).reshape(3) for c in crop)
    if out is None:
        out = torch.empty((total, 3), dtype=torch.float64, device=pts.device)
    if valid_out is None and (crop is not None or v8 is not None):
        valid_out = torch.empty((total,), dtype=torch.uint8, device=pts.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 3 * total
    assert valid_out is None or (valid_out.dtype == torch.uint8 and valid_out.is_contiguous() and valid_out.numel() == total)
    if total == 0:                                  # no rows, and a tensor without elements has no address to pass
        return out, valid_out
    _lib.check(lib.prg_rigid_crop_ragged_f64(_lib.ptr(pts), _lib.ptr(v8), _lib.ptr(offsets), B, total, _lib.ptr(Td),
                                             _lib.ptr(hd), None if lo is None else lo.ctypes.data, None if hi is None
                                             else hi.ctypes.data, _lib.ptr(out), _lib.ptr(valid_out), _lib.stream_ptr()),
               "prg_rigid_crop_ragged_f64")
    return out, valid_out


def augment_clouds(points: torch.Tensor, lengths, *, seeds, draw: int = 0, noise: float = 0.0, limit: Optional[int] = None,
                   T=None, has_T=None, keys=None):
    """prg_augment_ragged_f64: the registration loaders' augmentation of a stack of C clouds on the device — each cloud cut to
    `limit` rows by a keyed random permutation, moved by its 4x4, jittered by uniform noise inside (-noise/2, noise/2) — bit for
    bit `postprocess.augment_cloud` per cloud (which states the definition).  points (N,3) float64 or float32 device tensor
    (float32 is widened, which is exact), the clouds one after the other; lengths: their rows, a HOST list or array; seeds: C
    64-bit Philox keys (host ints, e.g. `synthetic.augment_seed`); draw: the second counter word — the epoch, for a job that
    re-augments cached pairs without regenerating them; T (C,4,4) float64 / has_T (C) as `rigid_crop_ragged` takes them; keys
    (N,) uint32 sort keys (numpy or int32 / uint32 tensor) instead of Philox's.
    -> {"points": (M,3) float64, "lengths": (C,) int64, "rows": (M,) int32 local input row of every output row}, all on the
    device, M = sum of min(n_c, limit).  Host synchronisations: none — the output offsets follow from `lengths` on
    the host, the small arrays are uploaded, one launch."""
    lib = _lib.load()
    if not points.is_cuda:
        raise _lib.PrgError("expected a tensor on the HIP device (this package has no CPU path)")
    if points.dtype not in (torch.float64, torch.float32):
        raise _lib.PrgError("augment_clouds: points must be float64 or float32")
    from .postprocess import _check_augment
    lim = _check_augment(noise, limit)
    if not 0 <= int(draw) < 2 ** 32:
        raise ValueError("draw must fit 32 bits")
    dev = points.device
    pts = points.contiguous().view(-1, 3).to(torch.float64)
    lens = np.asarray(lengths).astype(np.int64).reshape(-1)
    C = len(lens)
    if C < 1 or (lens < 0).any() or int(lens.sum()) != pts.shape[0]:
        raise ValueError("lengths do not add up to the rows of points")
    seeds = [int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]
    if len(seeds) != C:
        raise ValueError("one seed per cloud")
    m = np.minimum(lens, lim) if lim else lens.copy()
    offs, o_offs = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum(m)])
    total, M = int(offs[-1]), int(o_offs[-1])
    out = torch.empty((M, 3), dtype=torch.float64, device=dev)
    rows = torch.empty((M,), dtype=torch.int32, device=dev)
    res = {"points": out, "lengths": _dev_i64(m, dev), "rows": rows}
    if M == 0:                                      # no rows, and a tensor without elements has no address to pass
        return res
    kd = None
    if keys is not None:
        if not torch.is_tensor(keys):
            keys = torch.from_numpy(np.ascontiguousarray(keys).astype(np.uint32).view(np.int32))
        if keys.dtype == getattr(torch, "uint32", None):
            keys = keys.view(torch.int32)
        assert keys.dtype == torch.int32 and keys.numel() == total, "one 32-bit key per row"
        kd = keys.to(dev).contiguous()
    sd = torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)).to(dev)
    Td, hd = _transforms(T, C, dev), _flags(has_T, C, dev)
    d_offs, d_o_offs = _dev_i64(offs, dev), _dev_i64(o_offs, dev)        # named: both must be alive when the call is made
    _lib.check(lib.prg_augment_ragged_f64(_lib.ptr(pts), _lib.ptr(d_offs), C, total, _lib.ptr(Td), _lib.ptr(hd), _lib.ptr(sd),
                                          int(draw), _lib.ptr(kd), lim, float(noise), _lib.ptr(d_o_offs), M, _lib.ptr(out),
                                          _lib.ptr(rows), _lib.stream_ptr()), "prg_augment_ragged_f64")
    return res


def finish_clouds(pts: torch.Tensor, valid: Optional[torch.Tensor], offsets: torch.Tensor, voxel: float, *, pre=None,
                  has_pre=None, crop=None, post=None, has_post=None):
    """`WriterPool.cloud`'s pipeline for B ragged clouds at once, on the device: pre-transform -> crop -> voxel mean ->
    post-transform.  pts (total,3) float64, valid (total) bool / uint8 or None, offsets (B+1) int64, device tensors as for
    `voxel_grid_ragged`; pre / post: (B,4,4) float64 (numpy or tensor) or None, has_pre / has_post: (B) flags, None = every
    segment; crop: (lo, hi) or None.  Returns (out (rows,3) float64, out_offsets (B+1) int64, status (B) int32) on the device:
    out[out_offsets[b]:out_offsets[b+1]] is, bit for bit, the vertex payload of the PLY that `WriterPool.cloud(path, xyz_b,
    valid_b, pre=, crop=, voxel=, post=)` writes (`postprocess.finish_cloud` is the numpy form); status as `voxel_grid_ragged`.
    voxel <= 0 skips the grid: the kept rows stay in input order (compacted with torch on the device; that one path waits for
    the row count).  `pts` and `valid` are left as they are."""
    assert pts.dtype == torch.float64 and offsets.dtype == torch.int64
    pts = pts.contiguous().view(-1, 3)
    offsets = offsets.contiguous()
    total, B = pts.shape[0], offsets.numel() - 1
    cur, cur_valid = pts, _u8(valid)
    if pre is not None or crop is not None:
        # a crop alone moves nothing: the kernel then only writes the flags and `out` may be the input itself
        cur, cur_valid = rigid_crop_ragged(pts, cur_valid, offsets, T=pre, has_T=has_pre, crop=crop,
                                           out=pts if pre is None else None)
    if voxel > 0:
        out, out_offsets, status = voxel_grid_ragged(cur, cur_valid, offsets, voxel)
    else:
        idx = torch.arange(total, device=pts.device)
        keep = (idx >= offsets[0]) & (idx < offsets[-1])          # rows outside every segment hold nothing
        if cur_valid is not None:
            keep &= cur_valid != 0
        csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=pts.device), torch.cumsum(keep.to(torch.int64), 0)])
        out_offsets = csum[offsets.clamp(0, total)]
        out_offsets = out_offsets - out_offsets[0]
        out = cur[keep]
        status = torch.zeros((B,), dtype=torch.int32, device=pts.device)
    if post is not None and out.shape[0] > 0:
        rigid_crop_ragged(out, None, out_offsets, T=post, has_T=has_post, out=out)
    return out, out_offsets, status


def check_voxel_status(status, names: Sequence) -> None:
    """Raise PrgError naming the first scene whose voxel grid failed (`status` already on the host)."""
    for j, st in enumerate(np.asarray(status)):
        if st:
            raise _lib.PrgError("voxel_down_sample of {}: {}".format(
                names[j], "non-finite point" if st == 1 else "voxel_size is too small"))


def point_clouds(depth: torch.Tensor, intrinsic: torch.Tensor, pose: Optional[torch.Tensor] = None, *,
                 depth_unit: float = DEPTH_UNIT_M, clip=(0.5, 10.0)) -> List[np.ndarray]:
    """Per image: the compacted (n_valid,3) float64 cloud in row-major pixel order — what `point_cloud(img*10, K,
    clip)` followed by `(pc - t) @ R` returns in the reference (sd:2623-2628)."""
    xyz, valid = unproject_f64(depth, intrinsic, pose, depth_unit=depth_unit, clip=clip)
    xyz, valid = xyz.cpu().numpy(), valid.cpu().numpy()
    return [xyz[b][valid[b]] for b in range(xyz.shape[0])]


def depth_augment(depth: torch.Tensor) -> torch.Tensor:
    """DepthAugment (dc:577-604): (B,1,H,W) -> (B,3,H,W)."""
    lib = _lib.load()
    depth = _f32(depth)
    B, _, H, W = depth.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=depth.device)
    _lib.check(lib.prg_depth_augment(_lib.ptr(depth), _lib.ptr(out), B, H, W, _lib.stream_ptr()), "prg_depth_augment")
    return out


def apply_mask(prob: torch.Tensor, depth: torch.Tensor, hit: Optional[torch.Tensor], threshold: float = 0.99,
               want_cond: bool = True) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """keep = prob > thr; depth[~keep] = 0; hit &= keep; img_cond = cat[depth, hit]*2-1  (sd:2564-2570)."""
    lib = _lib.load()
    prob, depth = _f32(prob), _f32(depth)
    B, _, H, W = depth.shape
    h8 = _u8(hit)
    d_out = torch.empty_like(depth)
    h_out = torch.empty((B, 1, H, W), dtype=torch.uint8, device=depth.device)
    cond = torch.empty((B, 2, H, W), dtype=torch.float32, device=depth.device) if want_cond else None
    _lib.check(lib.prg_apply_mask(_lib.ptr(prob), _lib.ptr(depth), _lib.ptr(h8), float(threshold), _lib.ptr(d_out),
                                  _lib.ptr(h_out), _lib.ptr(cond), B, H, W, _lib.stream_ptr()), "prg_apply_mask")
    return d_out, h_out.view(torch.bool), cond


def occlusion_filter(depth_rpj: torch.Tensor, mask_rpj: torch.Tensor, threshold: float = 0.0375):
    """(sd:446-463) a reprojected pixel more than `threshold` metres behind the nearest valid depth of its 3x3 window
    takes that depth (thin foreground structures win over what shows through them).  Returns (depth, mask unchanged)."""
    lib = _lib.load()
    depth = _f32(depth_rpj)
    B, _, H, W = depth.shape
    m8 = _u8(mask_rpj)
    out = torch.empty_like(depth)
    _lib.check(lib.prg_occlusion_filter(_lib.ptr(depth), _lib.ptr(m8), _lib.ptr(out), B, H, W, float(threshold),
                                        _lib.stream_ptr()), "prg_occlusion_filter")
    return out, mask_rpj
