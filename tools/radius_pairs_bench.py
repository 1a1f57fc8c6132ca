#!/usr/bin/env python
"""What ground-truth correspondences cost on the device and on the host.  One GPU.  Writes
profiles/radius_pairs_bench.json.

Input: the finished cloud pairs of `--scenes` (256) synthetic scenes at `--size` (128) squared, as `PairStream` yields them
(bf16, dim 64, batch 64, the `--sampling-steps` sampler, synthetic weights) — the pairs that pass generate_gt's filter, in one
ragged float64 buffer on the device.  For each radius (0.0375, 0.05):

  count / fill   prg_radius_count_ragged_f64 (memset + sweep + scan) and prg_radius_fill_ragged_f64 on preallocated buffers, HIP
                 events around each call, median of `--repeats` (20) after 3 warm-up calls; K = the size of the list.  The first
                 pair's list is compared with the numpy specification first.
  nearest        prg_nearest_ragged_f64 on the same buffer, timed the same way.  It sweeps BOTH directions of every pair (rows of A
                 against B and rows of B against A), i.e. the all-pairs arithmetic twice; count + fill sweep one direction
                 twice.  So (count + fill) / nearest is expected near 1, and near 2 against half of nearest.
  host           scipy.spatial.cKDTree(tgt).query_ball_point(src, r, workers=min(16, usable CPUs)) per pair, build included:
                 what a loader's get_correspondences pays per item today (wall seconds over all pairs, median per pair).

Then pairs/s of `PairStream` (with matching_radius 0.0375, to="torch") against `generate(gt_log=True)` (one lane, default writer
pool, into a temporary folder that is removed) over the same scenes: each arm warmed on one batch, then timed alternately
`--wall-repeats` (2) times; host clock around work that ends in a device synchronise.

    python tools/radius_pairs_bench.py [--out profiles/radius_pairs_bench.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADII = (0.0375, 0.05)


def networks(a):
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.unet import MaskUnet, Unet
    unet = Unet(dim=a.dim, param_cond_dim=4, dim_mults=(1, 2, 4, 8), channels=1, dtype=a.dtype).init_synthetic(1)
    mask = MaskUnet(dim=a.dim, dim_mults=(1, 2, 4, 8), dtype=a.dtype).init_synthetic(2, final_bias=8.0)
    diff = GaussianDiffusion(unet, image_size=a.size, timesteps=1000, sampling_timesteps=a.sampling_steps, loss_type="l1",
                             objective="pred_x0", beta_schedule="sigmoid", ddim_sampling_eta=1.0, is_ddnm_sampling=True)
    return diff, mask


def timed(fn, repeats):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "repeats": repeats}


def kernel_leg(pairs, repeats):
    import torch
    from scipy.spatial import cKDTree

    from pointreggpt_amd import _lib
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    lib = _lib.load()
    clouds = [c for p in pairs for c in p]
    sizes = np.array([len(c) for c in clouds], dtype=np.int64)
    pts, offs = G.upload_clouds(clouds, "cuda", dtype=np.float64)
    total, n_pairs, max_cloud = pts.shape[0], len(pairs), int(sizes.max())
    ij = int((sizes[0::2] * sizes[1::2]).sum())                  # (row of A, row of B) tests of one sweep in one direction
    row_start = torch.empty((total + 1,), dtype=torch.int64, device="cuda")
    ws = torch.empty((int(lib.prg_radius_pairs_workspace_bytes(total)),), dtype=torch.uint8, device="cuda")
    d2 = torch.empty((total,), dtype=torch.float64, device="cuda")
    idx = torch.empty((total,), dtype=torch.int32, device="cuda")
    s = _lib.stream_ptr()

    def nearest():
        _lib.check(lib.prg_nearest_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), n_pairs, max_cloud, _lib.ptr(d2), _lib.ptr(idx), s))

    t_near = timed(nearest, repeats)
    workers = min(16, len(os.sched_getaffinity(0)))
    out = {"pairs": n_pairs, "rows_total": int(total), "rows_per_cloud_median": float(np.median(sizes)), "rows_per_cloud_max": max_cloud,
           "ij_tests_one_direction": ij, "nearest_both_directions": t_near, "host_workers": workers, "radii": []}
    for r in RADII:
        def count():
            _lib.check(lib.prg_radius_count_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), n_pairs, total, max_cloud, r, _lib.ptr(row_start),
                                                       _lib.ptr(ws), ws.numel(), s))
        count()
        K = int(row_start[total].item())
        corr = torch.empty((K, 2), dtype=torch.int32, device="cuda")

        def fill():
            _lib.check(lib.prg_radius_fill_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), n_pairs, max_cloud, r, _lib.ptr(row_start), K,
                                                      _lib.ptr(corr), s))
        fill()
        first = corr[:int(row_start[int(sizes[0] + sizes[1])].item())].cpu().numpy()
        if not np.array_equal(first, PP.radius_pairs(pairs[0][0], pairs[0][1], r)):
            raise SystemExit("the first pair's list differs from the numpy specification")
        t_count, t_fill = timed(count, repeats), timed(fill, repeats)
        both = t_count["ms_median"] + t_fill["ms_median"]
        per_pair, k_tree = [], 0
        t0 = time.perf_counter()
        for a, b in pairs:
            t1 = time.perf_counter()
            found = cKDTree(b).query_ball_point(a, r, workers=workers, return_length=True)
            per_pair.append(time.perf_counter() - t1)
            k_tree += int(found.sum())
        host_s = time.perf_counter() - t0
        row = {"radius": r, "K": K, "K_per_query_row": K / float(sizes[0::2].sum()), "count": t_count, "fill": t_fill,
               "count_plus_fill_ms": both, "count_plus_fill_over_nearest": both / t_near["ms_median"],
               "Gtests_per_s_count": ij / (t_count["ms_median"] * 1e-3) / 1e9, "Gtests_per_s_fill": ij / (t_fill["ms_median"] * 1e-3) / 1e9,
               "host_ckdtree_total_s": host_s, "host_ckdtree_ms_per_pair_median": 1e3 * statistics.median(per_pair),
               "host_ckdtree_K": k_tree, "device_ms_per_pair": both / n_pairs}
        print(json.dumps(row), flush=True)
        out["radii"].append(row)
        del corr
    return out


def rate_leg(a, diff, mask):
    import torch

    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.stream import PairStream
    tmp = tempfile.mkdtemp(prefix="radius_pairs_bench_", dir=a.workdir)

    def stream_arm(stop):
        gen = Generator(diff, None, batch_size=a.batch, samples_folder=os.path.join(tmp, "unused"), synthetic_seed=0)
        t0 = time.perf_counter()
        n = sum(1 for _ in PairStream(gen, mask, start=0, stop=stop, noise_seed=0, matching_radius=RADII[0], to="torch"))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, n

    def files_arm(stop):
        folder = os.path.join(tmp, "ds")
        gen = Generator(diff, None, batch_size=a.batch, samples_folder=os.path.join(folder, "data"), synthetic_seed=0)
        t0 = time.perf_counter()
        gen.generate(0, stop, 1, depth_correction=mask, noise_seed=0, gt_log=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        shutil.rmtree(folder)
        return dt, stop

    try:
        stream_arm(a.batch), files_arm(a.batch)                  # warm-up: one batch each
        res = {"stream_s": [], "files_s": []}
        yielded = None
        for _ in range(a.wall_repeats):
            dt, yielded = stream_arm(a.scenes)
            res["stream_s"].append(dt)
            res["files_s"].append(files_arm(a.scenes)[0])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    s_med, f_med = statistics.median(res["stream_s"]), statistics.median(res["files_s"])
    res.update(scenes=a.scenes, items_yielded=yielded, stream_scenes_per_s=a.scenes / s_med, files_scenes_per_s=a.scenes / f_med,
               what="wall seconds, host clock ending in a device synchronise, over the same scenes after one warm-up batch per arm, "
                    "alternated: PairStream(matching_radius=0.0375, to='torch') against generate(gt_log=True) with one lane and the "
                    "default writer pool (every file of the dataset written, then removed outside the timed window)")
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scenes", type=int, default=256)
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--dtype", default="bf16")
    p.add_argument("--sampling-steps", type=int, default=1000)
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--wall-repeats", type=int, default=2)
    p.add_argument("--no-rate", action="store_true", help="kernels and host only")
    p.add_argument("--workdir", default=None, help="where generate(gt_log=True) writes (default: the system's temporary folder)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_pairs_bench.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("radius_pairs_bench.py measures on the GPU: no HIP device visible")
    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.stream import PairStream
    res = {"device": torch.cuda.get_device_name(0), "host_cpus_usable": len(os.sched_getaffinity(0)),
           "config": {k: getattr(a, k) for k in ("scenes", "size", "batch", "dim", "dtype", "sampling_steps")}}
    diff, mask = networks(a)
    tmp = tempfile.mkdtemp(prefix="radius_pairs_bench_", dir=a.workdir)
    try:
        gen = Generator(diff, None, batch_size=a.batch, samples_folder=tmp, synthetic_seed=0)
        stream = PairStream(gen, mask, start=0, stop=a.scenes, noise_seed=0)
        pairs = [(it["src"], it["tgt"]) for it in stream]
        res["input"] = {"scenes": a.scenes, "pairs_after_the_gt_filter": len(pairs), "skipped": len(stream.skipped)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if not pairs:
        raise SystemExit("no pair passed generate_gt's filter: nothing to measure")
    print(json.dumps(res), flush=True)
    res["kernels"] = kernel_leg(pairs, a.repeats)
    if not a.no_rate:
        res["rate"] = rate_leg(a, diff, mask)
        print(json.dumps(res["rate"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
