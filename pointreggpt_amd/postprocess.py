"""Host post-processing of the generated views: crop, voxel-grid mean down-sampling, rigid transforms, PLY I/O and the
overlap ratio of `generate_gt.py` — what the reference delegates to open3d (sd:2484-2500, 2641-2680;
generate_gt.py:68-102).  open3d is not in this image, so these follow Open3D 0.17 semantics *as recalled from its
C++ source* and are **parity-unpinned** (DESIGN.md §2): crop bounds inclusive; voxel index =
floor((p - (min_bound - voxel/2)) / voxel), output = per-voxel mean (output order unspecified in open3d: here sorted
by voxel index, deterministic); PLY binary_little_endian with `double x y z`; radius search = any neighbour with
squared distance < r^2.

Two layers: the numpy forms below are the specification (and what the CPU tests compare with); `native_*` and `WriterPool`
run the same arithmetic in the library's C++ (csrc/hostpool.cpp, include/prg.h "Host post-processing") — the writer pool
produces a batch's files on worker threads while the GPU samples the next batch.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

BBOX_MIN = np.array([-1.5, -1.5, 0.5])    # sd:2348
BBOX_MAX = np.array([1.5, 1.5, 3.5])


def crop_aabb(pts: np.ndarray, lo=BBOX_MIN, hi=BBOX_MAX) -> np.ndarray:
    """PointCloud.crop(AxisAlignedBoundingBox): keep lo <= p <= hi (inclusive)."""
    pts = np.asarray(pts)
    if len(pts) == 0:
        return pts.reshape(0, 3)
    keep = np.all((pts >= lo) & (pts <= hi), axis=1)
    return pts[keep]


def transform(pts: np.ndarray, T: np.ndarray) -> np.ndarray:
    """PointCloud.transform(T): p' = R p + t, float64."""
    pts = np.asarray(pts, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    return pts @ T[:3, :3].T + T[:3, 3]


def voxel_down_sample(pts: np.ndarray, voxel_size: float) -> np.ndarray:
    """PointCloud.voxel_down_sample: mean of the points of every occupied voxel (float64), voxels in ascending key order, each
    mean = (sequential sum of its rows in input order) / count — bit for bit what the C++ and the device grid return."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    if len(pts) == 0:
        return pts
    if voxel_size <= 0:
        raise ValueError("voxel_size <= 0")
    origin = pts.min(axis=0) - voxel_size * 0.5
    idx = np.floor((pts - origin) / voxel_size).astype(np.int64)
    dims = idx.max(axis=0) + 1
    if float(dims[0]) * float(dims[1]) * float(dims[2]) >= 2 ** 62:
        raise ValueError("voxel_size is too small")          # open3d raises the same way
    key = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    order = np.argsort(key, kind="stable")
    key_s = key[order]
    starts = np.flatnonzero(np.r_[True, key_s[1:] != key_s[:-1]])
    counts = np.diff(np.r_[starts, len(key_s)])
    # the rows of a voxel are added ONE AFTER THE OTHER in input order, starting from the first (what csrc/hostpool.cpp and
    # csrc/voxelgrid.hip do): np.add.reduceat would add a run of 8 or more rows pairwise and differ from them in the last bits
    pts_s = pts[order]
    sums = pts_s[starts].copy()
    live = np.flatnonzero(counts > 1)
    k = 1
    while len(live):
        sums[live] += pts_s[starts[live] + k]
        k += 1
        live = live[counts[live] > k]
    return sums / counts[:, None]


def rigid_move(pts: np.ndarray, T: np.ndarray) -> np.ndarray:
    """p' = R p + t with every coordinate written out as x*T[r,0] + y*T[r,1] + z*T[r,2] + T[r,3], the products summed left to
    right in float64 — bit for bit csrc/hostpool.cpp's transform() and prg_rigid_crop_ragged_f64.  (`transform` above goes
    through the BLAS, which may fuse a product into the sum.)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty_like(pts)
    for r in range(3):
        out[:, r] = x * T[r, 0] + y * T[r, 1] + z * T[r, 2] + T[r, 3]
    return out


def finish_cloud(xyz: np.ndarray, valid: Optional[np.ndarray] = None, *, pre: Optional[np.ndarray] = None, crop: bool = True,
                 lo=BBOX_MIN, hi=BBOX_MAX, voxel: float = 0.025, post: Optional[np.ndarray] = None) -> np.ndarray:
    """The numpy specification of a finished cloud: the (n,3) float64 vertex payload of the PLY that
    `WriterPool.cloud(path, xyz, valid, pre=, crop=, voxel=, post=, lo=, hi=)` writes, bit for bit — rows with valid != 0 in
    input order -> pre (4x4, None = not moved: the rows are copied, never multiplied by an identity) -> crop to lo <= p <= hi
    (if crop) -> voxel mean (if voxel > 0) -> post.  What `geometry.finish_clouds` computes per segment on the device."""
    pts = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    if valid is not None:
        pts = pts[np.asarray(valid).reshape(-1) != 0]
    if pre is not None:
        pts = rigid_move(pts, pre)
    if crop:
        pts = crop_aabb(pts, np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
    if voxel > 0:
        pts = voxel_down_sample(pts, voxel)
    if post is not None:
        pts = rigid_move(pts, post)
    return np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------------
# PLY (what o3d.io.write_point_cloud / read_point_cloud exchange; the dataloaders only need the N x 3 points)
# ------------------------------------------------------------------------------------------------------------------
def write_ply(path: str, pts: np.ndarray) -> None:
    pts = np.ascontiguousarray(np.asarray(pts, dtype="<f8").reshape(-1, 3))
    header = ("ply\nformat binary_little_endian 1.0\ncomment Created by pointreggpt_amd\n"
              f"element vertex {len(pts)}\nproperty double x\nproperty double y\nproperty double z\nend_header\n")
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(pts.tobytes())
    os.replace(tmp, path)


_PLY_TYPES = {"double": "<f8", "float64": "<f8", "float": "<f4", "float32": "<f4", "uchar": "u1", "uint8": "u1",
              "char": "i1", "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
              "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}


def read_ply(path: str) -> np.ndarray:
    """(N,3) float64 points of a binary-little-endian or ascii PLY (vertex element, x/y/z properties)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, n, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated header")
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    n = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError("list properties on vertices are not supported")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        names = [p[0] for p in props]
        if not all(k in names for k in "xyz"):
            raise ValueError(f"{path}: vertex element lacks x/y/z")
        if fmt == "binary_little_endian":
            data = np.frombuffer(f.read(n * np.dtype(props).itemsize), dtype=np.dtype(props), count=n)
            return np.stack([data["x"], data["y"], data["z"]], axis=1).astype(np.float64)
        if fmt == "ascii":
            arr = np.loadtxt(f, max_rows=n, ndmin=2)
            return arr[:, [names.index("x"), names.index("y"), names.index("z")]].astype(np.float64)
        raise ValueError(f"{path}: unsupported PLY format {fmt}")


# ------------------------------------------------------------------------------------------------------------------
# overlap ratio (generate_gt.py:68-102) with a uniform grid instead of a per-point KD-tree loop
# ------------------------------------------------------------------------------------------------------------------
def _has_neighbour(query: np.ndarray, ref: np.ndarray, radius: float) -> np.ndarray:
    """bool[len(query)]: some ref point lies strictly within `radius` of the query point."""
    if len(query) == 0 or len(ref) == 0:
        return np.zeros(len(query), dtype=bool)
    cell = radius
    origin = np.minimum(query.min(0), ref.min(0)) - cell
    rc = np.floor((ref - origin) / cell).astype(np.int64)
    qc = np.floor((query - origin) / cell).astype(np.int64)
    dims = np.maximum(rc.max(0), qc.max(0)) + 2
    rkey = (rc[:, 0] * dims[1] + rc[:, 1]) * dims[2] + rc[:, 2]
    order = np.argsort(rkey, kind="stable")
    rkey_s, ref_s = rkey[order], ref[order]
    found = np.zeros(len(query), dtype=bool)
    r2 = radius * radius
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                todo = np.flatnonzero(~found)
                if len(todo) == 0:
                    return found
                c = qc[todo] + (dx, dy, dz)
                key = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
                lo = np.searchsorted(rkey_s, key, side="left")
                hi = np.searchsorted(rkey_s, key, side="right")
                # cells hold few points after the 0.025 voxel grid (cell 0.0375): walk them in lock step
                width = int((hi - lo).max()) if len(lo) else 0
                for k in range(width):
                    j = lo + k
                    ok = j < hi
                    jj = np.where(ok, j, 0)
                    d2 = ((ref_s[jj] - query[todo]) ** 2).sum(1)
                    hit = ok & (d2 < r2)
                    found[todo[hit]] = True
    return found


def compute_overlap_ratio(pc1: np.ndarray, pc2: np.ndarray, voxel_size: float = 0.025, overlap_factor: float = 1.5,
                          is_down_sample: bool = True) -> Tuple[float, float]:
    """Fraction of (down-sampled) points of each cloud with a neighbour of the other within 1.5 voxels."""
    if is_down_sample:
        pc1, pc2 = voxel_down_sample(pc1, voxel_size), voxel_down_sample(pc2, voxel_size)
    r = voxel_size * overlap_factor
    with np.errstate(invalid="ignore", divide="ignore"):
        o1 = np.float64(_has_neighbour(pc1, pc2, r).sum()) / np.float64(len(pc1))
        o2 = np.float64(_has_neighbour(pc2, pc1, r).sum()) / np.float64(len(pc2))
    return float(o1), float(o2)


# ------------------------------------------------------------------------------------------------------------------
# nearest point of another cloud and the distance metrics between two clouds (dataset comparison, compare.py)
# ------------------------------------------------------------------------------------------------------------------
DISTANCE_THRESHOLDS = (1e-4, 1e-3, 0.0125, 0.0375)   # north-star tolerance, 1 mm, half the save voxel, generate_gt's radius


def nearest(a: np.ndarray, b: np.ndarray, chunk: int = 1024) -> Tuple[np.ndarray, np.ndarray]:
    """For every row of `a`: (d2, idx) = the smallest squared distance to a row of `b` and the lowest row of `b` that attains
    it — the numpy specification of prg_nearest_ragged_f64, bit for bit.  d2 = dx*dx + dy*dy + dz*dz in float64 with the
    three products written out and summed left to right (as `rigid_move` writes its products out: nothing here goes through
    the BLAS or a pairwise sum).  A NaN never wins; a row with no finite candidate — `b` empty, NaN, or every distance
    overflowing — ends at +inf / -1.  The query rows are processed `chunk` at a time to bound the (chunk, len(b)) temporaries."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    d2 = np.full(len(a), np.inf, dtype=np.float64)
    idx = np.full(len(a), -1, dtype=np.int32)
    if len(a) == 0 or len(b) == 0:
        return d2, idx
    bx, by, bz = b[None, :, 0], b[None, :, 1], b[None, :, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(a), chunk):
            q = a[s:s + chunk]
            dx, dy, dz = bx - q[:, 0:1], by - q[:, 1:2], bz - q[:, 2:3]
            d = dx * dx + dy * dy + dz * dz
            d[np.isnan(d)] = np.inf
            j = np.argmin(d, axis=1)                      # the first occurrence of the minimum = the lowest row
            m = d[np.arange(len(q)), j]
            d2[s:s + chunk] = m
            idx[s:s + chunk] = np.where(np.isinf(m), -1, j)
    return d2, idx


def _pair_clouds(pairs):
    """[(a, b), ...] -> (clouds: the 2n float64 (rows,3) arrays in pair order, sizes (2n) int64, offs (2n+1) int64): the pair
    layout of prg_overlap_counts, on the host."""
    clouds = [_f64(c) for pair in pairs for c in pair]
    sizes = np.array([len(c) for c in clouds], dtype=np.int64)
    return clouds, sizes, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def nearest_hip(pairs, device="cuda"):
    """[(a (n,3), b (m,3)), ...] -> [(d2_ab, idx_ab, d2_ba, idx_ba), ...] as `nearest(a, b)` and `nearest(b, a)` define them:
    all clouds uploaded once as one ragged float64 buffer, ONE prg_nearest_ragged_f64 launch for the whole list."""
    from . import _lib
    from . import geometry as G
    _lib.load()
    _lib.require_gpu()
    if not pairs:
        return []
    clouds, sizes, offs = _pair_clouds(pairs)
    if sizes.max() == 0:
        d2 = np.full(0, np.inf)
        idx = np.full(0, -1, dtype=np.int32)
    else:
        pts, d_offs = G.upload_clouds(clouds, device, dtype=np.float64)
        d2_d, idx_d = G.nearest_ragged(pts, d_offs, len(pairs), int(sizes.max()))
        d2, idx = d2_d.cpu().numpy(), idx_d.cpu().numpy()
    out = []
    for p in range(len(pairs)):
        o0, o1, o2 = offs[2 * p], offs[2 * p + 1], offs[2 * p + 2]
        out.append((d2[o0:o1].copy(), idx[o0:o1].copy(), d2[o1:o2].copy(), idx[o1:o2].copy()))
    return out


def radius_pairs(a: np.ndarray, b: np.ndarray, radius: float, chunk: int = 1024) -> np.ndarray:
    """Every (i, j) with row j of `b` strictly within `radius` of row i of `a`, as a (K,2) int32 array ordered by i, then j — the
    numpy specification of prg_radius_count_ragged_f64 / prg_radius_fill_ragged_f64, bit for bit.  The test is `nearest`'s
    expression: dx*dx + dy*dy + dz*dz < radius*radius in float64 with dx = b.x - a.x, the products written out and summed left to
    right, so a row of `a` has matches iff `nearest(a, b)` gives it d2 < radius*radius, and its nearest row is among them.  A NaN
    row never matches; an empty `a` or `b` gives shape (0,2).  The query rows are processed `chunk` at a time, which bounds the
    (chunk, len(b)) temporaries and changes nothing else."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    r2 = np.float64(radius) * np.float64(radius)
    out = [np.zeros((0, 2), dtype=np.int32)]
    if len(a) and len(b):
        bx, by, bz = b[None, :, 0], b[None, :, 1], b[None, :, 2]
        with np.errstate(over="ignore", invalid="ignore"):
            for s in range(0, len(a), chunk):
                q = a[s:s + chunk]
                dx, dy, dz = bx - q[:, 0:1], by - q[:, 1:2], bz - q[:, 2:3]
                i, j = np.nonzero(dx * dx + dy * dy + dz * dz < r2)      # row-major: i ascending, then j
                out.append(np.stack([i + s, j], axis=1).astype(np.int32))
    return np.concatenate(out, axis=0)


def radius_pairs_hip(pairs, radius: float, device="cuda"):
    """[(a (n,3), b (m,3)), ...] -> [corr_p (K_p,2) int32, ...] as `radius_pairs(a, b, radius)` defines them, for clouds that
    are on the host (a loader's collate step on a batch of PLY pairs): all clouds uploaded once as one ragged float64 buffer,
    ONE count / fill (`geometry.radius_pairs_ragged`) for the whole list, one copy back."""
    from . import _lib
    from . import geometry as G
    _lib.load()
    _lib.require_gpu()
    if not pairs:
        return []
    clouds, sizes, _ = _pair_clouds(pairs)
    if sizes.max() == 0:
        return [np.zeros((0, 2), dtype=np.int32) for _ in pairs]
    pts, d_offs = G.upload_clouds(clouds, device, dtype=np.float64)
    corr_d, po_d = G.radius_pairs_ragged(pts, d_offs, len(pairs), int(sizes.max()), radius)
    corr, po = corr_d.cpu().numpy(), po_d.cpu().numpy()
    return [corr[po[p]:po[p + 1]].copy() for p in range(len(pairs))]


AUGMENT_TAG = 0x6175676D        # "augm": third Philox counter word of the augmentation stream, tag word of synthetic.augment_seed


def _check_augment(noise, limit) -> int:
    """-> limit as the entry point takes it (0 = all rows)."""
    if not (np.isfinite(noise) and noise >= 0):
        raise ValueError("noise must be finite and >= 0")
    if limit is not None and (int(limit) != limit or limit < 1):
        raise ValueError("limit must be a positive integer (or None for every row)")
    return 0 if limit is None else int(limit)


def augment_cloud(points: np.ndarray, *, seed: int, draw: int = 0, noise: float = 0.0, limit: Optional[int] = None,
                  T: Optional[np.ndarray] = None, keys: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """What the registration loaders do to a cloud before they search its correspondences — cut it to `limit` points by a
    random permutation, move it rigidly, add uniform noise — as a function of (seed, draw): the numpy specification of
    prg_augment_ragged_f64, bit for bit.  -> (points_out (m,3) float64, rows (m,) int32: which input row each output row was).

    Row i of the n input rows draws ONE Philox4x32-10 call, key `seed` (64 bits), counter {i, draw, 0x6175676D, 0} -> w0..w3.
    Selection: key_i = keys[i] (uint32) if `keys` is given, else w0; m = min(n, limit).  If m == n the rows keep their order
    (the loaders permute only when they cut).  Otherwise the rows are ordered by (key_i, i) and the first m are kept, in that
    order: a random permutation cut at m, like `np.random.permutation(n)[:limit]`.
    Position: `rigid_move(row, T)` if T is given (else the row's bits, -0.0 included), then, iff noise != 0, per axis a
    + (u - 0.5) * noise with u = (float64(w_{1+a}) + 0.5) * 2^-32: u and u - 0.5 are exact in float64, the product is the one
    rounding, and the noise lies strictly inside (-noise/2, noise/2) — the loaders' `(rand(n,3) - 0.5) * augment_noise`.  The
    noise of a row depends on (seed, draw, i) only, not on what the cut keeps."""
    from .philox import philox4x32_10
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    m = min(n, _check_augment(noise, limit) or n)
    if not 0 <= int(draw) < 2 ** 32:
        raise ValueError("draw must fit 32 bits")
    w = philox4x32_10(np.arange(n, dtype=np.uint64), int(draw), AUGMENT_TAG, 0, seed)
    if m == n:
        rows = np.arange(n, dtype=np.int32)
    else:
        key = w[0] if keys is None else np.asarray(keys).reshape(-1).astype(np.uint32)
        if len(key) != n:
            raise ValueError("one key per row")
        rows = np.lexsort((np.arange(n), key))[:m].astype(np.int32)          # by key, ties by row
    out = pts[rows] if T is None else rigid_move(pts[rows], T)
    if noise != 0.0:
        u = (np.stack(w[1:], axis=1)[rows].astype(np.float64) + 0.5) * 2.0 ** -32
        out = out + (u - 0.5) * np.float64(noise)
    return np.ascontiguousarray(out, dtype=np.float64).reshape(-1, 3), rows


def augment_clouds_hip(clouds, *, seeds, draw: int = 0, noise: float = 0.0, limit: Optional[int] = None, T=None, keys=None,
                       device="cuda"):
    """[cloud (n,3), ...] -> [(points_out, rows), ...] as `augment_cloud(cloud, seed=seeds[c], draw=, noise=, limit=, T=T[c],
    keys=keys[c])` defines them, for clouds that are on the host: all clouds uploaded once as one ragged float64 buffer, ONE
    prg_augment_ragged_f64 launch (`geometry.augment_clouds`), one copy back.  T: a list with a 4x4 or None per cloud, or None;
    keys: a list with a uint32 array per cloud, or None (Philox keys)."""
    from . import _lib
    from . import geometry as G
    _lib.load()
    _lib.require_gpu()
    clouds = [_f64(c) for c in clouds]
    if not clouds:
        return []
    if sum(len(c) for c in clouds) == 0:
        return [(np.zeros((0, 3)), np.zeros(0, dtype=np.int32)) for _ in clouds]
    pts, _ = G.upload_clouds(clouds, device, dtype=np.float64)
    has_T = Td = None
    if T is not None:
        has_T = np.array([t is not None for t in T], dtype=np.uint8)
        Td = np.stack([np.eye(4) if t is None else np.asarray(t, dtype=np.float64).reshape(4, 4) for t in T])
    kd = None
    if keys is not None:
        kd = np.concatenate([np.asarray(k).reshape(-1).astype(np.uint32) for k in keys])
    res = G.augment_clouds(pts, [len(c) for c in clouds], seeds=seeds, draw=draw, noise=noise, limit=limit, T=Td, has_T=has_T,
                           keys=kd)
    out, rows = res["points"].cpu().numpy(), res["rows"].cpu().numpy()
    o = np.concatenate([[0], np.cumsum([min(len(c), limit or len(c)) for c in clouds])])
    return [(out[o[c]:o[c + 1]].copy(), rows[o[c]:o[c + 1]].copy()) for c in range(len(clouds))]


def _fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fmaf(a, b, c) on float32 arrays, exactly: the product of two float32 is exact in float64; its sum with c is rounded to
    ODD there (TwoSum gives the error; an inexact even result moves one step towards the true value), and a 53-bit round-to-odd
    value rounds to float32 like the exact one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
    step = np.where((e > 0) == (s > 0), 1, -1).astype(np.int64)
    s = np.where(fix, (s.view(np.int64) + step).view(np.float64), s)
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def _se3_apply32(P: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """`pc @ R^T + t` as the kernels evaluate it (camera.h): per output j a float32 product, two fmaf in k order, one add."""
    P, pts = np.asarray(P, dtype=np.float32).reshape(4, 4), np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    out = np.empty_like(pts)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(3):
            v = pts[:, 0] * P[j, 0]
            v = _fma32(pts[:, 1], np.broadcast_to(P[j, 1], v.shape), v)
            v = _fma32(pts[:, 2], np.broadcast_to(P[j, 2], v.shape), v)
            out[:, j] = v + P[j, 3]
    return out


def pose_candidate_counts(clouds, poses, K, S, *, box=None, z_tol: float = 0.0375, box_frame: str = "target",
                          swap_rc: bool = False) -> np.ndarray:
    """THE definition of prg_pose_candidate_counts / prg_cpu_pose_candidate_counts in numpy: clouds [(n_b,3) float32, ...], poses
    (B,N,4,4) float32, K (B,3,3) float32, S the image size (an int, or (H, W)) -> counts (B,N,3) int32 = (in_frame, seen, covered)
    per (scene, candidate).  Every row p of cloud b is moved to q = R p + t by poses[b,c] in float32 (`_se3_apply32`) and
    projected like the z-buffer of `project_clouds`: the row is taken iff q.z > 0 (NaN fails) and col = rint(q.x*fx/q.z + cx),
    row = rint(q.y*fy/q.z + cy) (float32 throughout, round half to even) lie in [0, W) x [0, H).
      in_frame  the taken rows;
      covered   the pixels with a taken row;
      seen      the taken rows with float32 q.z <= zmin(pixel) + z_tol — zmin the smallest q.z of the pixel's taken rows, the sum
                in float32 — and, with box = (lo, hi), lo <= q <= hi componentwise in float32: the box is tested on the MOVED
                row, in the target camera frame, where the reference crops the target cloud (sd:2641-2650).
    `box_frame="source"` (the box on the unmoved row) and `swap_rc` (H and W exchanged in the frame test and the pixel index) are
    two wrong readings, kept for the tests that show a test set tells them apart."""
    poses, K = np.asarray(poses, dtype=np.float32), np.asarray(K, dtype=np.float32)
    H, W = (int(S), int(S)) if isinstance(S, (int, np.integer)) else (int(S[0]), int(S[1]))
    if swap_rc:
        H, W = W, H
    B, N = poses.shape[0], poses.shape[1]
    assert len(clouds) == B and poses.shape[2:] == (4, 4) and K.shape == (B, 3, 3)
    tol = np.float32(z_tol)
    lo = hi = None
    if box is not None:
        lo, hi = np.asarray(box[0], dtype=np.float32).reshape(3), np.asarray(box[1], dtype=np.float32).reshape(3)
    counts = np.zeros((B, N, 3), dtype=np.int32)
    for b in range(B):
        p = np.asarray(clouds[b], dtype=np.float32).reshape(-1, 3)
        fx, fy, cx, cy = K[b, 0, 0], K[b, 1, 1], K[b, 0, 2], K[b, 1, 2]
        for c in range(N):
            q = _se3_apply32(poses[b, c], p)
            x, y, z = q[:, 0], q[:, 1], q[:, 2]
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                fc, fr = np.rint(x * fx / z + cx), np.rint(y * fy / z + cy)
                take = (z > 0) & (fc >= 0) & (fc < np.float32(W)) & (fr >= 0) & (fr < np.float32(H))
            pix = fr[take].astype(np.int64) * W + fc[take].astype(np.int64)
            zt = z[take]
            zmin = np.full(H * W, np.inf, dtype=np.float32)
            np.minimum.at(zmin, pix, zt)
            with np.errstate(invalid="ignore"):
                seen = zt <= zmin[pix] + tol
            if lo is not None:
                r = (p if box_frame == "source" else q)[take]
                seen &= np.all((r >= lo) & (r <= hi), axis=1)
            counts[b, c] = (int(take.sum()), int(seen.sum()), len(np.unique(pix)))
    return counts


def pose_candidate_counts_hip(clouds, poses, K, S, *, box=None, z_tol: float = 0.0375, device="cuda", workspace_bytes=None):
    """`pose_candidate_counts` for clouds that are on the host, through the kernels: the clouds uploaded once as one ragged float32
    buffer, ONE prg_pose_candidate_counts call (`geometry.pose_candidate_counts`), one copy back -> (B,N,3) int32 numpy."""
    from . import _lib
    from . import geometry as G
    _lib.load()
    _lib.require_gpu()
    pts, offs = G.upload_clouds([np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds], device)
    return G.pose_candidate_counts(pts, offs, poses, K, S, box=box, z_tol=z_tol, workspace_bytes=workspace_bytes).cpu().numpy()


def _check_radius_limit(radius, limit) -> None:
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be finite and > 0")
    if int(limit) != limit or limit < 1:
        raise ValueError("limit must be an integer >= 1")


def radius_neighbors(a: np.ndarray, b: np.ndarray, radius: float, limit: int) -> Tuple[np.ndarray, np.ndarray]:
    """For every row of `a` its `limit` nearest rows of `b` within `radius`, nearest first: (idx (len(a), limit) int32, count
    (len(a),) int32) — the numpy specification of prg_radius_select_ragged_f64 on count / fill's list, bit for bit, and the
    neighbour table of a KPConv collate step.  The rows j that match row i are `radius_pairs`' (dx*dx + dy*dy + dz*dz <
    radius*radius in float64, dx = b.x - a.x, products written out and summed left to right, strict <); they are ordered by that
    squared distance ascending, then by j ascending; the first `limit` are kept and the remaining slots hold len(b), the index
    of the shadow row those networks append.  count[i] is the number of matches BEFORE truncation (what a neighbour limit is
    calibrated from).  A NaN row never matches and is never matched; an empty `a` gives shapes (0, limit) and (0,); an empty `b`
    gives all pads, and the pad is 0.  `limit` < 1, or a radius that is not finite and > 0, raises ValueError."""
    _check_radius_limit(radius, limit)
    limit = int(limit)
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    idx = np.full((len(a), limit), len(b), dtype=np.int32)
    corr = radius_pairs(a, b, radius)
    i, j = corr[:, 0].astype(np.int64), corr[:, 1].astype(np.int64)
    count = np.bincount(i, minlength=len(a)).astype(np.int32)
    if len(corr):
        dx, dy, dz = b[j, 0] - a[i, 0], b[j, 1] - a[i, 1], b[j, 2] - a[i, 2]
        d2 = dx * dx + dy * dy + dz * dz
        order = np.lexsort((j, d2, i))                               # by i, then d2, then j
        i, j = i[order], j[order]
        first = np.cumsum(count, dtype=np.int64) - count             # where row i's matches begin in the ordered list
        rank = np.arange(len(i), dtype=np.int64) - first[i]
        keep = rank < limit
        idx[i[keep], rank[keep]] = j[keep]
    return idx, count


def radius_neighbors_hip(pairs, radius: float, limit: int, device="cuda"):
    """[(a (n,3), b (m,3)), ...] -> [(idx_p (n,limit) int32, count_p (n,) int32), ...] as `radius_neighbors(a, b, radius, limit)`
    defines them, for clouds that are on the host: all clouds uploaded once as one ragged float64 buffer, ONE count / fill /
    select (`geometry.radius_neighbors_ragged`) for the whole list, one copy back."""
    from . import _lib
    from . import geometry as G
    _check_radius_limit(radius, limit)
    _lib.load()
    _lib.require_gpu()
    if not pairs:
        return []
    clouds, sizes, _ = _pair_clouds(pairs)
    pts, d_offs = G.upload_clouds(clouds, device, dtype=np.float64)
    table_d, to_d, count_d = G.radius_neighbors_ragged(pts, d_offs, len(pairs), max(1, int(sizes.max())), radius, int(limit))
    table, to, count = table_d.cpu().numpy(), to_d.cpu().numpy(), count_d.cpu().numpy()
    return [(table[to[p]:to[p + 1]].copy(), count[to[p]:to[p + 1]].copy()) for p in range(len(pairs))]


NORMALS_LANES = 8        # partial sums per row of estimate_normals (the lanes of a row in csrc/normals.hip)
NORMALS_SWEEPS = 6       # cyclic Jacobi sweeps (tests/test_normals_spec.py: a seventh changes no output bit on its inputs)


def _normals_sum(x: np.ndarray, k: np.ndarray) -> np.ndarray:
    """x (N, limit), k (N,) valid slots per row -> (N,): THE sum over the slots of estimate_normals.  NORMALS_LANES = 8 partial
    sums per row, each starting at +0.0; slot s < k is added to partial s mod 8, s ascending; the partials are combined by the
    tree ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).  Slots >= k are not part of it, whatever they hold."""
    part = np.zeros((x.shape[0], NORMALS_LANES), dtype=np.float64)
    for s in range(x.shape[1]):
        live = s < k
        if not live.any():
            break
        part[:, s % NORMALS_LANES] += np.where(live, x[:, s], 0.0)          # p + 0.0 == p, bit for bit: p is never -0.0
    pair = part[:, 0::2] + part[:, 1::2]
    quad = pair[:, 0::2] + pair[:, 1::2]
    return quad[:, 0] + quad[:, 1]


def _normals_rotate(A, V, p: int, q: int):
    """One Jacobi rotation of estimate_normals in the (p, q) plane, on rows where A[p][q] != 0; A: 3x3 nested lists of (N,)
    arrays kept symmetric, V: the same for the eigenvectors."""
    r = 3 - p - q
    apq = A[p][q]
    do = apq != 0.0
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    app, aqq = A[p][p] - h, A[q][q] + h
    apr, aqr = c * A[p][r] - s * A[q][r], s * A[p][r] + c * A[q][r]
    A[p][p], A[q][q] = np.where(do, app, A[p][p]), np.where(do, aqq, A[q][q])
    A[p][r] = A[r][p] = np.where(do, apr, A[p][r])
    A[q][r] = A[r][q] = np.where(do, aqr, A[q][r])
    A[p][q] = A[q][p] = np.where(do, 0.0, apq)
    for i in range(3):
        vp, vq = c * V[i][p] - s * V[i][q], s * V[i][p] + c * V[i][q]
        V[i][p], V[i][q] = np.where(do, vp, V[i][p]), np.where(do, vq, V[i][q])


def estimate_normals(points: np.ndarray, table: np.ndarray, count: np.ndarray, *, viewpoint=(0.0, 0.0, 0.0), min_neighbors: int = 3,
                     _sweeps: int = NORMALS_SWEEPS, _parts: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Oriented surface normals of a cloud from its neighbour table -> (normals (N,3) float64, variation (N,) float64): the
    numpy specification of prg_normals_ragged_f64, bit for bit.  points (N,3) float64; table (N, limit) int32 and count (N,) as
    `radius_neighbors(points, points, radius, limit)` returns them (pad slots hold N and are never read).  This function is the
    definition; every step is float64 arithmetic with +, -, *, / and sqrt only, no fused multiply-add, in exactly this order.

    Per row i, with k = min(count[i], limit) and the neighbours p_s = points[table[i, s]], s < k:
    1. Degenerate rows.  If k < min_neighbors, or a coordinate of points[i] is not finite: normal = (0, 0, 1) — open3d's
       convention —, variation = 0, and the row is not oriented.  Nothing below applies to it.
    2. Every "sum over the slots" below is `_normals_sum`: 8 partial sums from +0.0, slot s into partial s mod 8 in ascending s,
       combined as ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).
    3. Mean.  m = (sum x_s, sum y_s, sum z_s) / float(k), three divisions.
    4. Scatter matrix, a second pass.  d_s = p_s - m; S = the six sums of dx*dx, dx*dy, dx*dz, dy*dy, dy*dz, dz*dz (each product
       rounded, then summed).  S is not divided by k: neither output needs it.
    5. Eigen-decomposition of S by cyclic Jacobi, V = I: NORMALS_SWEEPS = 6 sweeps, each the rotations (p, q) = (0, 1), (0, 2),
       (1, 2) in this order, r the third index.  A rotation is done iff S_pq != 0:
         theta = (S_qq - S_pp) / (2 * S_pq);   t = sgn(theta) / (|theta| + sqrt(theta * theta + 1)), sgn(0) = +1 — an infinite
         theta, or a theta whose square overflows, gives t = 0 —;   c = 1 / sqrt(t * t + 1);   s = t * c;   h = t * S_pq;
         S_pp -= h;  S_qq += h;  (S_pr, S_qr) = (c * S_pr - s * S_qr, s * S_pr + c * S_qr);  S_pq = 0;
         for every row j of V: (V_jp, V_jq) = (c * V_jp - s * V_jq, s * V_jp + c * V_jq).
       Six sweeps: Jacobi converges quadratically and a 3x3 matrix with separated eigenvalues is diagonal to the last bit after
       four or five; tests/test_normals_spec.py checks that a seventh sweep changes no bit of either output on its inputs.
    6. Normal.  The column of V under the smallest diagonal entry of S, the lowest index on ties; NOT renormalised (its norm is 1
       to a few ulp).
    7. Variation.  lambda_min / ((S_00 + S_11) + S_22), 0 where that sum is 0.
    8. Orientation.  With v = viewpoint and p = points[i]: if (nx * (vx - px) + ny * (vy - py)) + nz * (vz - pz) < 0 the normal
       is negated; at exactly 0 it stays.

    `min_neighbors` < 3 raises ValueError.  (`_sweeps` and `_parts` are for the tests: another number of sweeps; a dict that
    receives "scatter", the (N,6) sums of step 4 — zeros on degenerate rows.)"""
    if int(min_neighbors) != min_neighbors or min_neighbors < 3:
        raise ValueError("min_neighbors must be an integer >= 3")
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    table = np.asarray(table)
    count = np.asarray(count).reshape(-1)
    if table.ndim != 2 or table.shape[0] != len(P) or len(count) != len(P) or table.shape[1] < 1:
        raise ValueError("table must be (len(points), limit) and count (len(points),)")
    v = np.asarray(viewpoint, dtype=np.float64).reshape(3)
    N, limit = table.shape
    normals = np.zeros((N, 3), dtype=np.float64)
    normals[:, 2] = 1.0
    variation = np.zeros((N,), dtype=np.float64)
    k = np.minimum(np.maximum(count.astype(np.int64), 0), limit)
    ok = (k >= int(min_neighbors)) & np.isfinite(P).all(axis=1)
    k = np.where(ok, k, 0)
    if _parts is not None:
        _parts["scatter"] = np.zeros((N, 6), dtype=np.float64)
    if not ok.any():
        return normals, variation
    with np.errstate(all="ignore"):
        valid = np.arange(limit)[None, :] < k[:, None]
        nb = P[np.where(valid, table, 0).astype(np.int64).clip(0, max(N - 1, 0))]          # (N, limit, 3); pad slots: any row
        kf = k.astype(np.float64)
        m = [_normals_sum(nb[:, :, a], k) / kf for a in range(3)]
        d = [nb[:, :, a] - m[a][:, None] for a in range(3)]
        S = {(a, b): _normals_sum(d[a] * d[b], k) for a in range(3) for b in range(a, 3)}
        if _parts is not None:
            _parts["scatter"][ok] = np.stack([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]], axis=1)[ok]
        A = [[S[min(a, b), max(a, b)].copy() for b in range(3)] for a in range(3)]
        V = [[np.full((N,), 1.0 if a == b else 0.0) for b in range(3)] for a in range(3)]
        for _ in range(int(_sweeps)):
            _normals_rotate(A, V, 0, 1)
            _normals_rotate(A, V, 0, 2)
            _normals_rotate(A, V, 1, 2)
        s1 = A[1][1] < A[0][0]
        l1 = np.where(s1, A[1][1], A[0][0])
        s2 = A[2][2] < l1
        lmin = np.where(s2, A[2][2], l1)
        n = [np.where(s2, V[a][2], np.where(s1, V[a][1], V[a][0])) for a in range(3)]
        total = (A[0][0] + A[1][1]) + A[2][2]
        var = np.where(total == 0.0, 0.0, lmin / total)
        dot = (n[0] * (v[0] - P[:, 0]) + n[1] * (v[1] - P[:, 1])) + n[2] * (v[2] - P[:, 2])
        flip = dot < 0.0
        n = np.stack([np.where(flip, -c, c) for c in n], axis=1)
    normals[ok] = n[ok]
    variation[ok] = var[ok]
    return normals, variation


def estimate_normals_cloud(points: np.ndarray, radius: float = 0.1, limit: int = 30, viewpoint=(0.0, 0.0, 0.0),
                           min_neighbors: int = 3) -> Tuple[np.ndarray, np.ndarray]:
    """`estimate_normals` on the cloud's own neighbour table: `radius_neighbors(points, points, radius, limit)` — per row its
    `limit` nearest rows within `radius`, itself included, open3d's KDTreeSearchParamHybrid(radius, max_nn=limit) — then the
    definition above.  -> (normals (N,3), variation (N,))."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    table, count = radius_neighbors(P, P, radius, limit)
    return estimate_normals(P, table, count, viewpoint=viewpoint, min_neighbors=min_neighbors)


def estimate_normals_hip(clouds, radius: float = 0.1, limit: int = 30, viewpoints=None, device="cuda"):
    """[cloud (n,3), ...] -> [(normals (n,3) float64, variation (n,) float64), ...] as `estimate_normals_cloud(cloud, radius,
    limit, viewpoints[c])` defines them, for clouds that are on the host: all clouds uploaded once as one float64 stack, ONE
    search and ONE kernel launch (`geometry.estimate_normals`) for the whole list, one copy back.  viewpoints: (len(clouds), 3)
    or None for the origin."""
    from . import _lib
    from . import geometry as G
    _check_radius_limit(radius, limit)
    _lib.load()
    _lib.require_gpu()
    if not len(clouds):
        return []
    clouds = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds]
    lens = [len(c) for c in clouds]
    pts, _ = G.upload_clouds(clouds, device, dtype=np.float64)
    normals, variation = G.estimate_normals(pts[:int(sum(lens))], lens, radius=radius, limit=limit, viewpoints=viewpoints, want_variation=True)
    normals, variation = normals.cpu().numpy(), variation.cpu().numpy()
    o = np.concatenate([[0], np.cumsum(lens)])
    return [(normals[o[c]:o[c + 1]].copy(), variation[o[c]:o[c + 1]].copy()) for c in range(len(clouds))]


def neighbor_pyramid(points: np.ndarray, lengths, num_stages: int, voxel_size: float, radius: float, neighbor_limits) -> dict:
    """The KPConv pyramid of a stack of C clouds, host specification of `geometry.neighbor_pyramid`, built from
    `radius_neighbors` and `voxel_down_sample` only.  points (N,3): the clouds one after the other, lengths (C,) their rows.
    Level 0 is the input stack, unchanged; level l+1 is `voxel_down_sample(cloud, voxel_size * 2**(l+1))` of every cloud of
    level l, re-stacked in cloud order.  With r_l = radius * 2**l:
      neighbors[l]    level l against itself,                   radius r_l,     limit neighbor_limits[l]
      subsampling[l]  query level l+1, candidates level l,      radius r_l,     limit neighbor_limits[l]      (l < num_stages - 1)
      upsampling[l]   query level l,   candidates level l+1,    radius 2 * r_l, limit neighbor_limits[l+1]    (l < num_stages - 1)
    Searches never cross clouds.  An index counts rows of the candidate level's STACK (cloud start + local j) and the pad is
    that level's total row count, the shadow row.  Returns {"points": [(N_l,3) float64], "lengths": [(C,) int64], "neighbors",
    "subsampling", "upsampling": [(rows, limit) int32], "counts": {"neighbors", "subsampling", "upsampling": [(rows,) int32]}}."""
    num_stages = int(num_stages)
    if num_stages < 1:
        raise ValueError("num_stages must be >= 1")
    limits = [int(k) for k in neighbor_limits]
    if len(limits) != num_stages:
        raise ValueError("one neighbor limit per stage")
    for k in limits:
        _check_radius_limit(radius, k)
    if not (np.isfinite(voxel_size) and voxel_size > 0):
        raise ValueError("voxel_size must be finite and > 0")
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lens.sum() != len(pts) or (lens < 0).any():
        raise ValueError("lengths do not add up to the rows of points")

    def split(p, n):
        o = np.concatenate([[0], np.cumsum(n)])
        return [p[o[c]:o[c + 1]] for c in range(len(n))], o

    def tables(query, q_lens, cand, c_lens, r, limit):
        qs, _ = split(query, q_lens)
        cs, co = split(cand, c_lens)
        idx, cnt = [np.zeros((0, limit), dtype=np.int32)], [np.zeros(0, dtype=np.int32)]
        for c in range(len(qs)):
            t, k = radius_neighbors(qs[c], cs[c], r, limit)
            hit = t < len(cs[c])
            t = np.where(hit, t + np.int32(co[c]), np.int32(len(cand))).astype(np.int32)
            idx.append(t)
            cnt.append(k)
        return np.concatenate(idx, 0), np.concatenate(cnt, 0)

    out = {"points": [pts], "lengths": [lens], "neighbors": [], "subsampling": [], "upsampling": [],
           "counts": {"neighbors": [], "subsampling": [], "upsampling": []}}
    for l in range(1, num_stages):
        clouds, _ = split(out["points"][-1], out["lengths"][-1])
        down = [voxel_down_sample(c, voxel_size * 2 ** l) for c in clouds]
        out["points"].append(np.concatenate([np.zeros((0, 3))] + down, 0))
        out["lengths"].append(np.array([len(d) for d in down], dtype=np.int64))
    for l in range(num_stages):
        r = radius * 2 ** l
        P, n = out["points"][l], out["lengths"][l]
        jobs = [("neighbors", P, n, P, n, r, limits[l])]
        if l < num_stages - 1:
            Pn, nn = out["points"][l + 1], out["lengths"][l + 1]
            jobs += [("subsampling", Pn, nn, P, n, r, limits[l]), ("upsampling", P, n, Pn, nn, 2 * r, limits[l + 1])]
        for name, q, ql, c, cl, rr, k in jobs:
            t, cnt = tables(q, ql, c, cl, rr, k)
            out[name].append(t)
            out["counts"][name].append(cnt)
    return out


def _check_patch_limit(limit) -> int:
    if int(limit) != limit or not 1 <= limit <= 256:
        raise ValueError("limit must be an integer in 1..256")
    return int(limit)


def node_patches(points: np.ndarray, nodes: np.ndarray, limit: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The point-to-node partition of a coarse-to-fine network and its inverse: (assign (n,) int32, table (m, limit) int32, sizes
    (m,) int32) — the numpy specification of prg_patch_tables_ragged on prg_nearest_ragged_f64's output, bit for bit.
    `d2, assign = nearest(points, nodes)`: every point belongs to its nearest node (dx*dx + dy*dy + dz*dz in float64, summed left
    to right; the lowest node row wins a tie); a NaN point, and every point when `nodes` is empty, gets -1 and is in no patch.
    sizes[k] is the number of points with assign == k.  Row k of table holds those points ordered by (d2 ascending, row ascending)
    — a strict total order, so the table is unique; the first `limit` are kept and the remaining slots hold n = len(points), the
    shadow row.  1 <= limit <= 256, else ValueError."""
    limit = _check_patch_limit(limit)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    nodes = np.asarray(nodes, dtype=np.float64).reshape(-1, 3)
    n, m = len(points), len(nodes)
    d2, assign = nearest(points, nodes)
    table = np.full((m, limit), n, dtype=np.int32)
    sizes = np.zeros(m, dtype=np.int32)
    live = np.flatnonzero(assign >= 0)
    if len(live):
        k = assign[live].astype(np.int64)
        sizes = np.bincount(k, minlength=m).astype(np.int32)
        order = np.lexsort((live, d2[live], k))                      # by node, then d2, then row
        k, i = k[order], live[order]
        first = np.cumsum(sizes, dtype=np.int64) - sizes             # where node k's members begin in the ordered list
        rank = np.arange(len(i), dtype=np.int64) - first[k]
        keep = rank < limit
        table[k[keep], rank[keep]] = i[keep]
    return assign, table, sizes


def patch_overlaps(src_points: np.ndarray, src_table: np.ndarray, tgt_points: np.ndarray, tgt_table: np.ndarray,
                   radius: float, chunk: int = 1 << 20) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Which node patches of two clouds overlap, and by how much: (node_corr (P,2) int32, hits (P,2) int32, overlap (P,) float64)
    — the numpy specification of prg_patch_overlap_ragged_f64 and of the Python layer on top of it, bit for bit.  Patch a of the
    source is the entries of src_table[a] that are not the pad len(src_points) (`node_patches`' table), patch b of the target
    likewise.  For every (a, b): hits_src = the points i of patch a that have a point j of patch b with dx*dx + dy*dy + dz*dz <
    radius*radius — `radius_pairs`' expression and strict <, float64, dx = tgt.x - src.x, products written out and summed left to
    right — and hits_tgt = the points j of patch b that have such an i.  node_corr lists every (a, b) with hits_src > 0 (which is
    hits_tgt > 0) ordered by a, then b; hits its (hits_src, hits_tgt); overlap = (hits_src / |patch a| + hits_tgt / |patch b|) / 2
    with float64 division and addition in exactly this order.  A NaN row never matches.  The target nodes are processed in blocks
    of about `chunk` distance tests per source node, which bounds the temporaries and changes nothing else."""
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be finite and > 0")
    a = np.asarray(src_points, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(tgt_points, dtype=np.float64).reshape(-1, 3)
    ta, tb = np.asarray(src_table, dtype=np.int64), np.asarray(tgt_table, dtype=np.int64)
    if ta.ndim != 2 or tb.ndim != 2:
        raise ValueError("patch tables must be (nodes, limit)")
    ms, mt = len(ta), len(tb)
    in_a, in_b = ta != len(a), tb != len(b)
    r2 = np.float64(radius) * np.float64(radius)
    bp = np.full((mt, tb.shape[1], 3), np.nan)                        # the target patches' points, NaN in the pad slots
    bp[in_b] = b[tb[in_b]]
    hs, ht = np.zeros((ms, mt), dtype=np.int32), np.zeros((ms, mt), dtype=np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(ms):
            q = a[ta[s][in_a[s]]]
            if not len(q) or not mt:
                continue
            step = max(1, int(chunk) // max(1, len(q) * tb.shape[1]))
            for t in range(0, mt, step):
                c = bp[None, t:t + step]
                dx, dy, dz = c[..., 0] - q[:, None, None, 0], c[..., 1] - q[:, None, None, 1], c[..., 2] - q[:, None, None, 2]
                w = dx * dx + dy * dy + dz * dz < r2                  # (points of patch a, target nodes, slots of patch b)
                hs[s, t:t + step] = w.any(axis=2).sum(axis=0)
                ht[s, t:t + step] = w.any(axis=0).sum(axis=1)
    A, B = np.nonzero(hs > 0)                                         # row-major: a ascending, then b
    hits = np.stack([hs[A, B], ht[A, B]], axis=1).astype(np.int32)
    size_a, size_b = in_a.sum(axis=1).astype(np.float64), in_b.sum(axis=1).astype(np.float64)
    overlap = (hits[:, 0].astype(np.float64) / size_a[A] + hits[:, 1].astype(np.float64) / size_b[B]) / np.float64(2)
    return np.stack([A, B], axis=1).astype(np.int32), hits, overlap


def coarse_ground_truth(pyramid: dict, *, fine_level: int, limit: int, radius: float) -> dict:
    """The patch-level ground truth of a coarse-to-fine network from a `neighbor_pyramid` whose stack is [src_0, tgt_0, src_1,
    tgt_1, ...] (an even number of clouds; item p is clouds 2p and 2p+1): host specification of `geometry.coarse_ground_truth`.
    The nodes are the last level, the fine points level `fine_level` (0 <= fine_level < num_stages; with the last level every
    node is its own patch).  Per cloud `node_patches(fine points, nodes, limit)`, per item `patch_overlaps(..., radius)` of its
    two clouds.  Returns {"assign": (N_f,) int32 — per fine point its node as a row of the node level's STACK, -1 for none;
    "table": (M, limit) int32 — per node its patch as rows of the fine level's stack, the pad is N_f, the level's row count,
    exactly as the pyramid's neighbour tables are indexed; "sizes": (M,) int32; "node_corr": (P,2) int32 — (source node, target
    node) as rows of the node level's stack, ordered by item, then source, then target; "hits": (P,2) int32; "overlap": (P,)
    float64; "corr_offsets": (items+1,) int64 — item p's pairs are rows [corr_offsets[p], corr_offsets[p+1])}."""
    limit = _check_patch_limit(limit)
    levels = len(pyramid["points"])
    if int(fine_level) != fine_level or not 0 <= fine_level < levels:
        raise ValueError("fine_level must be in 0..num_stages-1")
    fine = np.asarray(pyramid["points"][int(fine_level)], dtype=np.float64).reshape(-1, 3)
    nodes = np.asarray(pyramid["points"][-1], dtype=np.float64).reshape(-1, 3)
    fl = np.asarray(pyramid["lengths"][int(fine_level)], dtype=np.int64).reshape(-1)
    nl = np.asarray(pyramid["lengths"][-1], dtype=np.int64).reshape(-1)
    if len(fl) % 2 or len(fl) != len(nl):
        raise ValueError("the stack must hold an even number of clouds: [src_0, tgt_0, src_1, tgt_1, ...]")
    fo, no = np.concatenate([[0], np.cumsum(fl)]), np.concatenate([[0], np.cumsum(nl)])
    assign, table, sizes, local = [np.zeros(0, np.int32)], [np.zeros((0, limit), np.int32)], [np.zeros(0, np.int32)], []
    for c in range(len(fl)):
        a, t, s = node_patches(fine[fo[c]:fo[c + 1]], nodes[no[c]:no[c + 1]], limit)
        local.append(t)
        assign.append(np.where(a >= 0, a + np.int32(no[c]), np.int32(-1)).astype(np.int32))
        table.append(np.where(t < fl[c], t + np.int32(fo[c]), np.int32(len(fine))).astype(np.int32))
        sizes.append(s)
    corr, hits, overlap, co = [np.zeros((0, 2), np.int32)], [np.zeros((0, 2), np.int32)], [np.zeros(0)], [0]
    for p in range(len(fl) // 2):
        s, t = 2 * p, 2 * p + 1
        nc, h, o = patch_overlaps(fine[fo[s]:fo[s + 1]], local[s], fine[fo[t]:fo[t + 1]], local[t], radius)
        corr.append((nc + np.array([no[s], no[t]], dtype=np.int32)).astype(np.int32))
        hits.append(h)
        overlap.append(o)
        co.append(co[-1] + len(nc))
    return {"assign": np.concatenate(assign), "table": np.concatenate(table, 0), "sizes": np.concatenate(sizes),
            "node_corr": np.concatenate(corr, 0), "hits": np.concatenate(hits, 0), "overlap": np.concatenate(overlap),
            "corr_offsets": np.asarray(co, dtype=np.int64)}


def patch_corr_labels(points: np.ndarray, table: np.ndarray, pairs: np.ndarray, radius: float, chunk: int = 1 << 22) -> np.ndarray:
    """The fine-level ground truth of a coarse-to-fine network: per selected patch pair the (K+1, K+1) label matrix of its
    optimal-transport loss, (S, K+1, K+1) bool — the numpy specification of prg_patch_corr_labels_f64, bit for bit.
    `points` (N,3) float64 is the fine level's stack, `table` (M,K) int32 the patches as rows of that stack (`coarse_ground_truth`'s
    "table"; an entry outside [0, N) is a pad, and the valid slots need not form a prefix), `pairs` (S,2) int32 rows of `table` as
    (a, b) = (source node, target node).  With i = table[a, u] and j = table[b, v]: labels[s, u, v] = both slots valid and
    dx*dx + dy*dy + dz*dz < radius*radius — `radius_pairs`' expression and strict <, float64, dx = points[j].x - points[i].x,
    products written out and summed left to right; labels[s, u, K] = slot u valid and row u holds no match; labels[s, K, v] =
    slot v valid and column v holds no match; labels[s, K, K] = False.  Validity is by index only: a valid slot that points at a
    NaN row matches nothing, so its slack label is True.  A pair whose a or b lies outside [0, M) stands for two empty patches:
    its matrix is all False.  1 <= K <= 256, radius finite and > 0, else ValueError.  The pairs are processed in blocks of about
    `chunk` distance tests, which bounds the temporaries and changes nothing else."""
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be finite and > 0")
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    tab = np.asarray(table, dtype=np.int64)
    if tab.ndim != 2:
        raise ValueError("the patch table must be (nodes, limit)")
    K = _check_patch_limit(tab.shape[1])
    prs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n, m, S = len(pts), len(tab), len(prs)
    labels = np.zeros((S, K + 1, K + 1), dtype=bool)
    if S == 0 or m == 0:
        return labels
    valid = (tab >= 0) & (tab < n)
    pp = np.full((m, K, 3), np.nan)                                   # the patches' points, NaN in the pad slots
    pp[valid] = pts[tab[valid]]
    r2 = np.float64(radius) * np.float64(radius)
    real = ((prs >= 0) & (prs < m)).all(axis=1)
    step = max(1, int(chunk) // (K * K))
    with np.errstate(over="ignore", invalid="ignore"):
        for s0 in range(0, S, step):
            sel = np.flatnonzero(real[s0:s0 + step]) + s0
            if not len(sel):
                continue
            a, b = prs[sel, 0], prs[sel, 1]
            A, B = pp[a][:, :, None, :], pp[b][:, None, :, :]
            dx, dy, dz = B[..., 0] - A[..., 0], B[..., 1] - A[..., 1], B[..., 2] - A[..., 2]
            w = dx * dx + dy * dy + dz * dz < r2                      # (pairs, slots of patch a, slots of patch b)
            labels[sel, :K, :K] = w
            labels[sel, :K, K] = valid[a] & ~w.any(axis=2)
            labels[sel, K, :K] = valid[b] & ~w.any(axis=1)
    return labels


def select_node_corr(overlap: np.ndarray, corr_offsets: np.ndarray, keys: np.ndarray, *, min_overlap: float,
                     num_targets: int) -> Tuple[np.ndarray, np.ndarray]:
    """Which ground-truth node pairs a coarse-to-fine consumer trains its fine level on: (rows (S,) int64, sel_offsets (items+1,)
    int64) — host specification of `geometry.select_node_corr`.  The candidates of item p are the rows r in [corr_offsets[p],
    corr_offsets[p+1]) with overlap[r] > min_overlap (strict); an item with more than `num_targets` candidates keeps the
    `num_targets` with the smallest (keys[r], r) — with independent uniform keys a uniform sample without replacement.  `rows` is
    ascending within each item, the items in order; item p's rows are rows[sel_offsets[p]:sel_offsets[p+1]].  keys is (P,)
    float64; num_targets >= 1, else ValueError."""
    if int(num_targets) != num_targets or num_targets < 1:
        raise ValueError("num_targets must be an integer >= 1")
    ov = np.asarray(overlap, dtype=np.float64).reshape(-1)
    co = np.asarray(corr_offsets, dtype=np.int64).reshape(-1)
    ky = np.asarray(keys, dtype=np.float64).reshape(-1)
    if len(ky) != len(ov):
        raise ValueError("one key per listed node pair")
    rows, so = [np.zeros(0, dtype=np.int64)], [0]
    for p in range(len(co) - 1):
        r = np.arange(co[p], co[p + 1], dtype=np.int64)
        r = r[ov[r] > min_overlap]
        if len(r) > num_targets:
            r = np.sort(r[np.lexsort((r, ky[r]))[:int(num_targets)]])
        rows.append(r)
        so.append(so[-1] + len(r))
    return np.concatenate(rows), np.asarray(so, dtype=np.int64)


def fine_ground_truth(pyramid: dict, gt: dict, *, fine_level: int, radius: float, keys, min_overlap: float = 0.1,
                      num_targets: int = 128) -> dict:
    """The fine-level ground truth of a coarse-to-fine network from a `neighbor_pyramid` and the `coarse_ground_truth` dict `gt`
    of the same `fine_level`: host specification of `geometry.fine_ground_truth`.  `select_node_corr(gt["overlap"],
    gt["corr_offsets"], keys, ...)` picks the node pairs, `patch_corr_labels(points[fine_level], gt["table"], node_corr, radius)`
    labels them.  Returns {"rows": (S,) int64 — indices into gt["node_corr"]; "sel_offsets": (items+1,) int64; "node_corr": (S,2)
    int32 = gt["node_corr"][rows]; "src_table", "tgt_table": (S,K) int32 = gt["table"] at the two columns of node_corr;
    "src_mask", "tgt_mask": (S,K) bool — True where the table entry is not the pad; "labels": (S,K+1,K+1) bool}."""
    levels = len(pyramid["points"])
    if int(fine_level) != fine_level or not 0 <= fine_level < levels:
        raise ValueError("fine_level must be in 0..num_stages-1")
    fine = np.asarray(pyramid["points"][int(fine_level)], dtype=np.float64).reshape(-1, 3)
    table = np.asarray(gt["table"], dtype=np.int32)
    rows, sel_offsets = select_node_corr(gt["overlap"], gt["corr_offsets"], keys, min_overlap=min_overlap, num_targets=num_targets)
    node_corr = np.asarray(gt["node_corr"], dtype=np.int32).reshape(-1, 2)[rows]
    src_table, tgt_table = table[node_corr[:, 0]], table[node_corr[:, 1]]
    return {"rows": rows, "sel_offsets": sel_offsets, "node_corr": node_corr, "src_table": src_table, "tgt_table": tgt_table,
            "src_mask": src_table != len(fine), "tgt_mask": tgt_table != len(fine),
            "labels": patch_corr_labels(fine, table, node_corr, radius)}


def patch_corr_labels_hip(points, table, pairs, radius: float, device="cuda") -> np.ndarray:
    """`patch_corr_labels(points, table, pairs, radius)` for arrays that are on the host: uploaded once, ONE
    `geometry.patch_corr_labels`, one copy back."""
    import torch

    from . import _lib
    from . import geometry as G
    _lib.load()
    _lib.require_gpu()
    tab = np.ascontiguousarray(table, dtype=np.int32)
    if tab.ndim != 2:
        raise ValueError("the patch table must be (nodes, limit)")
    up = lambda a: torch.tensor(a, device=device)                                # noqa: E731 (a copy: `a` may be read-only)
    labels = G.patch_corr_labels(up(_f64(points)), up(tab), up(np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)), radius)
    return labels.cpu().numpy()


def node_patches_hip(clouds, limit: int, device="cuda"):
    """[(points (n,3), nodes (m,3)), ...] -> [(assign, table, sizes), ...] as `node_patches(points, nodes, limit)` defines them,
    for clouds that are on the host: everything uploaded once, ONE `geometry.node_patches_ragged` for the whole list, one copy
    back."""
    import torch

    from . import _lib
    from . import geometry as G
    limit = _check_patch_limit(limit)
    _lib.load()
    _lib.require_gpu()
    if not clouds:
        return []
    pts, nds = [_f64(p) for p, _ in clouds], [_f64(q) for _, q in clouds]
    po = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
    no = np.concatenate([[0], np.cumsum([len(q) for q in nds])]).astype(np.int64)
    up = lambda rows: torch.from_numpy(np.concatenate(rows, 0)).to(device)       # noqa: E731
    assign_d, table_d, sizes_d = G.node_patches_ragged(up(pts), po, up(nds), no, limit)
    assign, table, sizes = assign_d.cpu().numpy(), table_d.cpu().numpy(), sizes_d.cpu().numpy()
    return [(assign[po[c]:po[c + 1]].copy(), table[no[c]:no[c + 1]].copy(), sizes[no[c]:no[c + 1]].copy())
            for c in range(len(clouds))]


def patch_overlaps_hip(items, radius: float, device="cuda", prefilter: bool = True):
    """[(src_points, src_table, tgt_points, tgt_table), ...] -> [(node_corr, hits, overlap), ...] as `patch_overlaps` defines them,
    for clouds and tables that are on the host: everything uploaded once, ONE `geometry.patch_overlaps_ragged` for the whole
    list, one copy back.  All tables must have the same number of columns."""
    import torch

    from . import _lib
    from . import geometry as G
    _lib.load()
    _lib.require_gpu()
    if not items:
        return []
    clouds = [_f64(c) for it in items for c in (it[0], it[2])]
    tabs = [np.ascontiguousarray(t, dtype=np.int32) for it in items for t in (it[1], it[3])]
    limit = _check_patch_limit(tabs[0].shape[1])
    if any(t.ndim != 2 or t.shape[1] != limit for t in tabs):
        raise ValueError("all patch tables must be (nodes, limit) with one limit")
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    toffs = np.concatenate([[0], np.cumsum([len(t) for t in tabs])]).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(clouds, 0)).to(device)
    tables = torch.from_numpy(np.concatenate(tabs, 0)).to(device)
    corr_d, hits_d, ov_d, co_d = G.patch_overlaps_ragged(pts, offs, tables, toffs, radius, prefilter=prefilter)
    corr, hits, ov, co = corr_d.cpu().numpy(), hits_d.cpu().numpy(), ov_d.cpu().numpy(), co_d.cpu().numpy()
    return [(corr[co[p]:co[p + 1]].copy(), hits[co[p]:co[p + 1]].copy(), ov[co[p]:co[p + 1]].copy()) for p in range(len(items))]


def cloud_distance_metrics(d2_ab: np.ndarray, d2_ba: np.ndarray, thresholds=DISTANCE_THRESHOLDS) -> dict:
    """Distances between two clouds from the squared nearest-neighbour distances of both directions (host float64, over
    d = sqrt(d2)): n_a, n_b, chamfer = (mean d_ab + mean d_ba) / 2, hausdorff = the largest d, p50 / p95 / p99 of all the
    distances of both directions together (np.percentile), within[t] = the share of those distances <= t.  If either cloud
    is empty there is nothing to measure: every metric is NaN and empty = True."""
    d_ab = np.sqrt(np.asarray(d2_ab, dtype=np.float64).reshape(-1))
    d_ba = np.sqrt(np.asarray(d2_ba, dtype=np.float64).reshape(-1))
    thresholds = tuple(float(t) for t in thresholds)
    m = {"n_a": int(len(d_ab)), "n_b": int(len(d_ba)), "empty": len(d_ab) == 0 or len(d_ba) == 0}
    if m["empty"]:
        nan = float("nan")
        m.update(chamfer=nan, hausdorff=nan, p50=nan, p95=nan, p99=nan, within={t: nan for t in thresholds})
        return m
    both = np.concatenate([d_ab, d_ba])
    p50, p95, p99 = np.percentile(both, [50, 95, 99])
    m.update(chamfer=float((d_ab.mean() + d_ba.mean()) / 2), hausdorff=float(both.max()), p50=float(p50), p95=float(p95),
             p99=float(p99), within={t: float((both <= t).mean()) for t in thresholds})
    return m


# ------------------------------------------------------------------------------------------------------------------
# image side files (torchvision.utils.save_image / cv2.imwrite equivalents; real-data parity unpinned)
# ------------------------------------------------------------------------------------------------------------------
def save_image01(img01: np.ndarray, path: str) -> None:
    """utils.save_image of a (1,H,W) or (H,W) tensor in [0,1]: x*255 + 0.5, clamp, uint8, grey replicated to RGB."""
    from PIL import Image
    a = np.asarray(img01, dtype=np.float32)
    a = a.reshape(a.shape[-2], a.shape[-1])
    u8 = np.clip(a * 255.0 + 0.5, 0, 255).astype(np.uint8)
    Image.fromarray(np.stack([u8] * 3, axis=-1), mode="RGB").save(path)


def save_depth16(depth01: np.ndarray, path: str) -> None:
    """cv2.imwrite(path, (depth * 1e4).astype(uint16)) (sd:2618-2620): 0.1 mm units... of the 10 m-normalised depth."""
    from PIL import Image
    a = np.asarray(depth01, dtype=np.float32)
    a = a.reshape(a.shape[-2], a.shape[-1])
    Image.fromarray((a * 1e4).astype(np.uint16)).save(path)


# ------------------------------------------------------------------------------------------------------------------
# native (C++) forms: csrc/hostpool.cpp behind the C-ABI
# ------------------------------------------------------------------------------------------------------------------
def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def _dp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def native_voxel_down_sample(pts, voxel_size: float) -> np.ndarray:
    from . import _lib
    lib = _lib.load()
    p = _f64(pts)
    out = np.empty_like(p)
    n = C.c_int64(0)
    _lib.check(lib.prg_host_voxel_down_sample(_dp(p), len(p), float(voxel_size), _dp(out), C.byref(n)),
               "prg_host_voxel_down_sample")
    return out[:n.value].copy()


def native_crop_aabb(pts, lo=BBOX_MIN, hi=BBOX_MAX) -> np.ndarray:
    from . import _lib
    lib = _lib.load()
    p = _f64(pts)
    out = np.empty_like(p)
    n = C.c_int64(0)
    lo64, hi64 = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    _lib.check(lib.prg_host_crop_aabb(_dp(p), len(p), _dp(lo64), _dp(hi64), _dp(out), C.byref(n)), "prg_host_crop_aabb")
    return out[:n.value].copy()


def native_write_ply(path: str, pts) -> None:
    from . import _lib
    p = _f64(pts)
    _lib.check(_lib.load().prg_host_write_ply(os.fsencode(path), _dp(p), len(p)), "prg_host_write_ply")


def rank_cpu_budget() -> int:
    """CPUs this rank may count on: the affinity mask when sharding.pin_rank_cpus narrowed it to this rank's private share (it
    leaves the marker PRG_PINNED_CPUS), otherwise the CPUs the process may use — the whole host, or a container cpuset / job-wide
    taskset that EVERY rank shares — divided by the ranks of the job (LOCAL_WORLD_SIZE, else WORLD_SIZE)."""
    total = os.cpu_count() or 4
    mine = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else total
    pinned = os.environ.get("PRG_PINNED_CPUS", "")
    if pinned.isdigit() and int(pinned) == mine:
        return max(1, mine)
    ranks = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    return max(1, mine // max(1, ranks))


class WriterPool:
    """Asynchronous per-scene output (prg_pool_*): every submit copies its inputs and returns at once; `wait()` blocks
    until all files exist and raises on the first failed job."""

    def __init__(self, threads: int = 0):
        from . import _lib
        self._lib = _lib
        lib = _lib.load()
        if threads <= 0:
            threads = max(2, min(16, rank_cpu_budget() // 2))
        self.threads = threads
        self._h = C.c_void_p()
        _lib.check(lib.prg_pool_create(int(threads), C.byref(self._h)), "prg_pool_create")

    def cloud(self, path: str, xyz: np.ndarray, valid: Optional[np.ndarray] = None, *, pre: Optional[np.ndarray] = None,
              crop: bool = True, voxel: float = 0.025, post: Optional[np.ndarray] = None, lo=BBOX_MIN, hi=BBOX_MAX):
        """xyz (n,3) float64 [valid (n,) bool] -> pre (4x4) -> crop -> voxel mean -> post (4x4) -> PLY at `path`."""
        p = _f64(xyz)
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        t0 = None if pre is None else np.ascontiguousarray(pre, dtype=np.float64)
        t1 = None if post is None else np.ascontiguousarray(post, dtype=np.float64)
        lo64, hi64 = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        self._lib.check(self._lib.load().prg_pool_submit_cloud(self._h, os.fsencode(path), _dp(p), len(p), _dp(v), _dp(t0),
                                                               int(crop), _dp(lo64), _dp(hi64), float(voxel), _dp(t1)),
                        "prg_pool_submit_cloud")

    def image01(self, path: str, img: np.ndarray):
        a = np.ascontiguousarray(np.asarray(img, dtype=np.float32).reshape(img.shape[-2], img.shape[-1]))
        self._lib.check(self._lib.load().prg_pool_submit_image(self._h, os.fsencode(path), _dp(a), a.shape[0], a.shape[1], 0))

    def depth16(self, path: str, img: np.ndarray):
        a = np.ascontiguousarray(np.asarray(img, dtype=np.float32).reshape(img.shape[-2], img.shape[-1]))
        self._lib.check(self._lib.load().prg_pool_submit_image(self._h, os.fsencode(path), _dp(a), a.shape[0], a.shape[1], 1))

    def text(self, path: str, values: np.ndarray):
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(values, dtype=np.float64)))
        self._lib.check(self._lib.load().prg_pool_submit_text(self._h, os.fsencode(path), _dp(a), a.shape[0], a.shape[1]))

    def wait(self) -> int:
        n = C.c_int64(0)
        self._lib.check(self._lib.load().prg_pool_wait(self._h, C.byref(n)), "prg_pool_wait")
        return int(n.value)

    def close(self):
        if self._h:
            self._lib.load().prg_pool_destroy(self._h)
            self._h = C.c_void_p()

    # `with WriterPool() as pool:` — leaving the block normally waits for every file and raises the first worker error;
    # leaving it on an exception lets the already queued jobs finish (nothing is half-written), reports a worker error
    # on stderr without masking the original exception, and tears the pool down.  Callers submit a batch's resume marker
    # only after `wait()` succeeded, so an aborted run never leaves a marker behind.
    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        worker_error = None
        try:
            if self._h:
                self.wait()
        except Exception as e:          # noqa: BLE001 — surfaced below
            worker_error = e
        self.close()
        if worker_error is not None:
            if exc_type is None:
                raise worker_error
            import sys
            print(f"writer pool: a queued job also failed while unwinding: {worker_error}", file=sys.stderr)
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------------------------
# overlap ratios on the GPU (generate_gt.py:68-102): voxel grids of all clouds in one ragged device call (or one by one in
# C++ on the host), neighbour-existence counts in one HIP launch
# ------------------------------------------------------------------------------------------------------------------
def overlap_ratios_hip(pairs, voxel_size: float = 0.025, overlap_factor: float = 1.5, is_down_sample: bool = True,
                       device="cuda", voxel: str = "device"):
    """[(src (n,3), tgt (m,3)), ...] -> [(overlap_src, overlap_tgt), ...] exactly as compute_overlap_ratio defines them:
    both clouds voxel-down-sampled, then the fraction of points with a point of the other cloud strictly within
    overlap_factor * voxel_size.  One prg_overlap_counts launch for the whole list (float64 all-pairs test).
    `voxel`: "device" = all clouds uploaded once and down-sampled by one prg_voxel_grid_ragged call whose output feeds the
    count kernel in place; "host" = each cloud through the C++ grid on the calling thread, then uploaded.  Same ratios."""
    import torch

    from . import _lib
    lib = _lib.load()
    _lib.require_gpu()
    if voxel not in ("device", "host"):
        raise ValueError("voxel must be 'device' or 'host'")
    if not pairs:
        return []
    if voxel == "device" and is_down_sample:
        from . import geometry as G
        raw = [_f64(c) for pair in pairs for c in pair]
        in_max = max(len(c) for c in raw)
        if in_max == 0:
            return [(float("nan"), float("nan"))] * len(pairs)
        pts, d_offs = G.upload_clouds(raw, device, dtype=np.float64)
        down, down_offs, status = G.voxel_grid_ragged(pts, None, d_offs, voxel_size)
        counts = torch.empty((len(pairs), 2), dtype=torch.int32, device=device)
        # max_cloud bounds the query slabs per cloud: the largest INPUT cloud is an upper bound of the largest down-sampled one
        _lib.check(lib.prg_overlap_counts(_lib.ptr(down), _lib.ptr(down_offs), len(pairs), int(in_max),
                                          float(voxel_size * overlap_factor), _lib.ptr(counts), _lib.stream_ptr()),
                   "prg_overlap_counts")
        G.check_voxel_status(status.cpu().numpy(), ["cloud {} of pair {}".format(k % 2, k // 2) for k in range(len(raw))])
        sizes = np.diff(down_offs.cpu().numpy())
        cnt = counts.cpu().numpy().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return [(float(cnt[i, 0] / np.float64(sizes[2 * i])), float(cnt[i, 1] / np.float64(sizes[2 * i + 1])))
                    for i in range(len(pairs))]
    clouds, sizes, offs = _pair_clouds([tuple(native_voxel_down_sample(c, voxel_size) if is_down_sample else c for c in pair)
                                        for pair in pairs])
    if offs[-1] == 0 or sizes.max() == 0:
        return [(float("nan"), float("nan"))] * len(pairs)
    pts = torch.from_numpy(np.concatenate([c for c in clouds if len(c)], axis=0)).to(device)
    d_offs = torch.from_numpy(offs).to(device)
    counts = torch.empty((len(pairs), 2), dtype=torch.int32, device=device)
    _lib.check(lib.prg_overlap_counts(_lib.ptr(pts), _lib.ptr(d_offs), len(pairs), int(sizes.max()),
                                      float(voxel_size * overlap_factor), _lib.ptr(counts), _lib.stream_ptr()),
               "prg_overlap_counts")
    cnt = counts.cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return [(float(cnt[i, 0] / np.float64(sizes[2 * i])), float(cnt[i, 1] / np.float64(sizes[2 * i + 1])))
                for i in range(len(pairs))]


def overlap_ratios_indexed_hip(clouds, pairs, voxel_size: float = 0.025, overlap_factor: float = 1.5, voxel: str = "device",
                               device="cuda"):
    """`overlap_ratios_hip` for pairs that share clouds: clouds = [(n,3), ...], pairs = [(s, t), ...] indices into it ->
    [(overlap of cloud s, overlap of cloud t), ...] per pair, exactly as `compute_overlap_ratio(clouds[s], clouds[t])` defines
    them.  Every cloud is uploaded and voxel-down-sampled ONCE, however many pairs it is in (`voxel` as in `overlap_ratios_hip`),
    and the pairs go through prg_overlap_counts_indexed, 65535 per launch."""
    import torch

    from . import _lib
    from . import geometry as G
    _lib.load()
    _lib.require_gpu()
    if voxel not in ("device", "host"):
        raise ValueError("voxel must be 'device' or 'host'")
    pairs = [(int(s), int(t)) for s, t in pairs]
    if any(not (0 <= s < len(clouds) and 0 <= t < len(clouds)) for s, t in pairs):
        raise ValueError("a pair names a cloud that is not in the list")
    if not pairs:
        return []
    raw = [_f64(c) for c in clouds]
    if voxel == "host":
        raw = [native_voxel_down_sample(c, voxel_size) for c in raw]
    in_max = max(len(c) for c in raw)
    if in_max == 0:
        return [(float("nan"), float("nan"))] * len(pairs)
    pts, d_offs = G.upload_clouds(raw, device, dtype=np.float64)
    if voxel == "device":
        pts, d_offs, status = G.voxel_grid_ragged(pts, None, d_offs, voxel_size)
    index = torch.from_numpy(np.array(pairs, dtype=np.int32).reshape(-1, 2)).to(pts.device)
    # max_cloud bounds the query slabs per cloud: the largest INPUT cloud is an upper bound of the largest down-sampled one
    counts = torch.cat([G.overlap_counts_indexed(pts, d_offs, index[k:k + 65535], in_max, voxel_size * overlap_factor)
                        for k in range(0, len(pairs), 65535)], dim=0)
    if voxel == "device":
        G.check_voxel_status(status.cpu().numpy(), ["cloud {}".format(k) for k in range(len(raw))])
        sizes = np.diff(d_offs.cpu().numpy())
    else:
        sizes = np.array([len(c) for c in raw], dtype=np.int64)
    cnt = counts.cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return [(float(cnt[i, 0] / np.float64(sizes[s])), float(cnt[i, 1] / np.float64(sizes[t]))) for i, (s, t) in enumerate(pairs)]
