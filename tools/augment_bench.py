#!/usr/bin/env python
"""What the loaders' augmentation costs on the device.  One GPU.  Writes profiles/augment_bench.json.

Input: `--clouds` (250) voxel-like clouds of ~4.5 k rows (tools/neighbor_tables_bench.py's), the size and density of the
generator's finished clouds, in one ragged float64 buffer on the device; every cloud has a rigid move; noise 0.005.

  (a) nothing cut         prg_augment_ragged_f64, limit 0: the streaming case, 24 B in and 28 B out per row; and the same call
                          with noise 0, which draws nothing: what the Philox call per row costs
  (b) every cloud halved  limit = half the smallest cloud: every cloud ranks its rows (the LDS sweep), then writes `limit` rows
  rigid crop              prg_rigid_crop_ragged_f64 alone on the same buffer and matrices: the streaming ceiling (24 B in, 24 B out)
  torch                   the formulation a user writes today, on the same device: per cloud `randperm(n)[:limit]` (case b),
                          `@ R.T + t`, `+ (rand(n,3) - 0.5) * noise`.  A different program (unseeded, one launch sequence per
                          cloud), not the code under test.

HIP events around each call on preallocated buffers, median of `--repeats` (20) after 3 warm-up calls.  The first and the last
cloud of both cases are compared with the numpy specification first.

    python tools/augment_bench.py [--out profiles/augment_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from neighbor_tables_bench import timed, voxel_like  # noqa: E402

NOISE = 0.005


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--clouds", type=int, default=250)
    p.add_argument("--rows", type=int, default=4500)
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench.py measures on the GPU: no HIP device visible")
    from scipy.spatial.transform import Rotation

    from pointreggpt_amd import _lib
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    lib = _lib.load()
    C = a.clouds
    rng = np.random.default_rng(C)
    clouds = [voxel_like(rng, int(n)) for n in rng.integers(int(a.rows * 0.8), int(a.rows * 1.2) + 1, size=C)]
    sizes = np.array([len(c) for c in clouds], dtype=np.int64)
    T = np.tile(np.eye(4), (C, 1, 1))
    T[:, :3, :3] = Rotation.random(C, random_state=1).as_matrix()
    T[:, :3, 3] = rng.standard_normal((C, 3))
    seeds = [int(s) for s in rng.integers(0, 2 ** 63, size=C)]
    pts, offs = G.upload_clouds(clouds, "cuda", dtype=np.float64)
    total = int(sizes.sum())
    half = int(sizes.min()) // 2
    Td = torch.from_numpy(T).cuda().view(C, 16)
    sd = torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)).cuda()
    out = torch.empty((total, 3), dtype=torch.float64, device="cuda")
    rows = torch.empty((total,), dtype=torch.int32, device="cuda")
    o_half = torch.arange(C + 1, dtype=torch.int64, device="cuda") * half
    s = _lib.stream_ptr()

    def augment(limit, o_offs, o_total, noise=NOISE):
        _lib.check(lib.prg_augment_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), C, total, _lib.ptr(Td), None, _lib.ptr(sd), 0, None,
                                              limit, noise, _lib.ptr(o_offs), o_total, _lib.ptr(out), _lib.ptr(rows), s))

    def crop():
        _lib.check(lib.prg_rigid_crop_ragged_f64(_lib.ptr(pts), None, _lib.ptr(offs), C, total, _lib.ptr(Td), None, None, None,
                                                 _lib.ptr(out), None, s))

    h_offs = np.concatenate([[0], np.cumsum(sizes)])
    for limit, o_offs, o_total, step in ((0, offs, total, None), (half, o_half, C * half, half)):
        augment(limit, o_offs, o_total)
        for c in (0, C - 1):
            want, want_rows = PP.augment_cloud(clouds[c], seed=seeds[c], noise=NOISE, limit=limit or None, T=T[c])
            o0 = int(h_offs[c]) if step is None else c * step
            if not (np.array_equal(out[o0:o0 + len(want)].cpu().numpy().view(np.uint64), want.view(np.uint64)) and
                    np.array_equal(rows[o0:o0 + len(want)].cpu().numpy(), want_rows)):
                raise SystemExit("cloud {} differs from the numpy specification (limit {})".format(c, limit))

    Rt = [torch.from_numpy(T[c, :3, :3].T.copy()).cuda() for c in range(C)]
    tt = [torch.from_numpy(T[c, :3, 3].copy()).cuda() for c in range(C)]
    views = [pts[int(h_offs[c]):int(h_offs[c + 1])] for c in range(C)]

    def torch_user(limit):
        res = []
        for c in range(C):
            x = views[c]
            if limit:
                x = x[torch.randperm(x.shape[0], device="cuda")[:limit]]
            res.append(x @ Rt[c] + tt[c] + (torch.rand(x.shape, dtype=torch.float64, device="cuda") - 0.5) * NOISE)
        return res

    t_a = timed(lambda: augment(0, offs, total), a.repeats)
    t_a0 = timed(lambda: augment(0, offs, total, 0.0), a.repeats)
    t_b = timed(lambda: augment(half, o_half, C * half), a.repeats)
    t_crop = timed(crop, a.repeats)
    t_torch_a = timed(lambda: torch_user(0), a.repeats)
    t_torch_b = timed(lambda: torch_user(half), a.repeats)
    gbs = lambda nbytes, t: nbytes / (t["ms_median"] * 1e-3) / 1e9
    res = {"device": torch.cuda.get_device_name(0), "clouds": C, "rows": total, "rows_per_cloud_median": float(np.median(sizes)),
           "rows_per_cloud_max": int(sizes.max()), "noise": NOISE, "limit_b": half,
           "key_comparisons_b": int((sizes * sizes).sum()),
           "a_nothing_cut": dict(t_a, bytes=52 * total, gb_per_s=gbs(52 * total, t_a)),
           "a_without_noise": dict(t_a0, bytes=52 * total, gb_per_s=gbs(52 * total, t_a0)),
           "b_every_cloud_halved": dict(t_b, rows_out=C * half),
           "rigid_crop_alone": dict(t_crop, bytes=48 * total, gb_per_s=gbs(48 * total, t_crop)),
           "torch_a": t_torch_a, "torch_b": t_torch_b,
           "a_ms_over_rigid_crop_ms": t_a["ms_median"] / t_crop["ms_median"],
           "a_gb_per_s_over_rigid_crop_gb_per_s": gbs(52 * total, t_a) / gbs(48 * total, t_crop),
           "torch_a_over_a": t_torch_a["ms_median"] / t_a["ms_median"],
           "torch_b_over_b": t_torch_b["ms_median"] / t_b["ms_median"]}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
