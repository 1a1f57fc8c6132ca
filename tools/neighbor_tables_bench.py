#!/usr/bin/env python
"""What a KPConv neighbour table costs on the device and on the host.  One GPU.  Writes
profiles/neighbor_tables_bench.json.

Input: `--pairs` (16 and 250) pairs of voxel-like clouds of ~4.5 k rows — a 2.5 cm grid surface patch with a few millimetres of
jitter, and the same patch moved by a centimetre of noise and permuted: the density and the size of a finished pair of the
generator, without running the networks.  Every cloud is searched against ITSELF (the neighbours table of a
pyramid level: pair p = the cloud twice), in one ragged float64 buffer on the device.  For each (radius, limit) of (0.0625, 38) —
the first level of the consumers' configuration — and (0.125, 38) — the second level's radius at the first level's density, i.e.
four times the matches per row:

  count / fill / select   prg_radius_count_ragged_f64, prg_radius_fill_ragged_f64 and prg_radius_select_ragged_f64 on preallocated
                          buffers, HIP events around each call, median of `--repeats` (20) after 3 warm-up calls; K = the size of
                          the list, the share of truncated rows.  The first pair's table is compared with the numpy specification
                          first.
  host                    scipy.spatial.cKDTree(cloud).query_ball_point(cloud, r, workers=min(16, usable CPUs)) per cloud, build
                          included, then per row the sort by (distance, index) and the cut at `limit` — the same table (wall seconds,
                          over at most `--host-pairs` (16) clouds, scaled to all of them).

    python tools/neighbor_tables_bench.py [--out profiles/neighbor_tables_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = ((0.0625, 38), (0.125, 38))


def voxel_like(rng, n):
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 0.025
    a = np.concatenate([g, 1.5 + 0.1 * np.sin(3 * g[:, :1])], 1) + rng.uniform(-0.004, 0.004, (n, 3))
    return a[rng.permutation(n)]


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


def host_table(cloud, r, limit, workers):
    """The same table from scipy: ball query, then per row the order (squared distance, index) and the cut."""
    from scipy.spatial import cKDTree
    n = len(cloud)
    found = cKDTree(cloud).query_ball_point(cloud, r, workers=workers)
    table = np.full((n, limit), n, dtype=np.int32)
    for i, js in enumerate(found):
        js = np.sort(np.asarray(js, dtype=np.int64))
        d = cloud[js] - cloud[i]
        js = js[np.argsort(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], kind="stable")][:limit]
        table[i, :len(js)] = js
    return table


def leg(n_pairs, rows, repeats, host_pairs):
    import torch

    from pointreggpt_amd import _lib
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    lib = _lib.load()
    rng = np.random.default_rng(n_pairs)
    clouds = [voxel_like(rng, int(n)) for n in rng.integers(int(rows * 0.8), int(rows * 1.2) + 1, size=n_pairs)]
    sizes = np.array([len(c) for c in clouds], dtype=np.int64)
    pts, offs = G.upload_clouds([c for c in clouds for _ in range(2)], "cuda", dtype=np.float64)
    total, max_cloud, Q = pts.shape[0], int(sizes.max()), int(sizes.sum())
    row_start = torch.empty((total + 1,), dtype=torch.int64, device="cuda")
    ws = torch.empty((int(lib.prg_radius_pairs_workspace_bytes(total)),), dtype=torch.uint8, device="cuda")
    t_offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)])).cuda()
    s = _lib.stream_ptr()
    workers = min(16, len(os.sched_getaffinity(0)))
    out = {"pairs": n_pairs, "query_rows": Q, "rows_per_cloud_median": float(np.median(sizes)), "rows_per_cloud_max": max_cloud,
           "ij_tests_per_sweep": int((sizes * sizes).sum()), "host_workers": workers, "settings": []}
    for r, limit in SETTINGS:
        def count():
            _lib.check(lib.prg_radius_count_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), n_pairs, total, max_cloud, r, _lib.ptr(row_start),
                                                       _lib.ptr(ws), ws.numel(), s))
        count()
        K = int(row_start[total].item())
        corr = torch.empty((K, 2), dtype=torch.int32, device="cuda")
        table = torch.empty((Q, limit), dtype=torch.int32, device="cuda")

        def fill():
            _lib.check(lib.prg_radius_fill_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), n_pairs, max_cloud, r, _lib.ptr(row_start), K,
                                                      _lib.ptr(corr), s))

        def select():
            _lib.check(lib.prg_radius_select_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), n_pairs, max_cloud, _lib.ptr(row_start),
                                                        _lib.ptr(corr), K, limit, _lib.ptr(t_offs), None, None, _lib.ptr(table), s))
        fill()
        select()
        want, cnt = PP.radius_neighbors(clouds[0], clouds[0], r, limit)
        if not np.array_equal(table[:len(clouds[0])].cpu().numpy(), want):
            raise SystemExit("the first cloud's table differs from the numpy specification")
        t_count, t_fill, t_select = timed(count, repeats), timed(fill, repeats), timed(select, repeats)
        rs = row_start.cpu().numpy()
        m = np.concatenate([np.diff(rs[o:o + n + 1]) for o, n in zip(offs.cpu().numpy()[0::2], sizes)])
        device_ms = t_count["ms_median"] + t_fill["ms_median"] + t_select["ms_median"]
        n_host = min(host_pairs, n_pairs)
        per_cloud = []
        for c in clouds[:n_host]:
            t0 = time.perf_counter()
            got = host_table(c, r, limit, workers)
            per_cloud.append(time.perf_counter() - t0)
        if not np.array_equal(got, table[int(sizes[:n_host - 1].sum()):int(sizes[:n_host].sum())].cpu().numpy()):
            raise SystemExit("scipy's table differs from the device's")
        host_ms = 1e3 * sum(per_cloud) * (Q / float(sizes[:n_host].sum()))
        row = {"radius": r, "limit": limit, "K": K, "matches_per_row_mean": float(m.mean()), "matches_per_row_max": int(m.max()),
               "rows_truncated_share": float((m > limit).mean()), "count": t_count, "fill": t_fill, "select": t_select,
               "device_ms": device_ms, "device_ms_per_cloud": device_ms / n_pairs,
               "select_share": t_select["ms_median"] / device_ms, "host_clouds_timed": n_host,
               "host_ms_per_cloud_median": 1e3 * statistics.median(per_cloud), "host_ms_all_clouds_scaled": host_ms,
               "host_over_device": host_ms / device_ms}
        print(json.dumps(row), flush=True)
        out["settings"].append(row)
        del corr, table
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, nargs="+", default=[16, 250])
    p.add_argument("--rows", type=int, default=4500)
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--host-pairs", type=int, default=16)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_tables_bench.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("neighbor_tables_bench.py measures on the GPU: no HIP device visible")
    res = {"device": torch.cuda.get_device_name(0), "host_cpus_usable": len(os.sched_getaffinity(0)), "legs": []}
    for n in a.pairs:
        res["legs"].append(leg(n, a.rows, a.repeats, a.host_pairs))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
