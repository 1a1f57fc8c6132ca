#!/usr/bin/env python
"""What oriented normals cost on the device.  One GPU.  Writes profiles/normals_bench.json.

Input: one batch of `--pairs` (64) synthetic pairs, i.e. 128 voxel-like clouds of ~4.5 k rows (tools/neighbor_tables_bench.py's
2.5 cm grid surface patch with a few millimetres of jitter: the density and size of a finished cloud of the generator), each
searched against itself in one ragged float64 buffer, at `stream.Normals`' defaults radius 0.1 and limit 30.

  count / fill / select   the search, on preallocated buffers, HIP events around each call
  normals                 prg_normals_ragged_f64 on select's table, with and without the variation output
each the median of `--repeats` (20) after 3 warm-up calls.  The first cloud's normals are compared with the numpy specification
first.  `layer_ms`: `geometry.estimate_normals` end to end (the cat, the search with its read-back, the kernel), host clock
around a device synchronise.

    python tools/normals_bench.py [--out profiles/normals_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

RADIUS, LIMIT = 0.1, 30


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, default=64)
    p.add_argument("--rows", type=int, default=4500)
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("normals_bench.py measures on the GPU: no HIP device visible")
    from neighbor_tables_bench import timed, voxel_like

    from pointreggpt_amd import _lib
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    lib = _lib.load()
    C = 2 * a.pairs
    rng = np.random.default_rng(a.pairs)
    clouds = [voxel_like(rng, int(n)) for n in rng.integers(int(a.rows * 0.8), int(a.rows * 1.2) + 1, size=C)]
    sizes = np.array([len(c) for c in clouds], dtype=np.int64)
    o = np.concatenate([[0], np.cumsum(sizes)])
    stack, d_o = G.upload_clouds(clouds, "cuda", dtype=np.float64)
    pts, offs = G.upload_clouds([c for c in clouds for _ in range(2)], "cuda", dtype=np.float64)
    total, max_cloud, Q = pts.shape[0], int(sizes.max()), int(sizes.sum())
    row_start = torch.empty((total + 1,), dtype=torch.int64, device="cuda")
    ws = torch.empty((int(lib.prg_radius_pairs_workspace_bytes(total)),), dtype=torch.uint8, device="cuda")
    base = torch.from_numpy(o[:C].astype(np.int32)).cuda()
    views = torch.from_numpy(rng.uniform(-3.0, 3.0, (C, 3))).cuda()
    s = _lib.stream_ptr()

    def count():
        _lib.check(lib.prg_radius_count_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), C, total, max_cloud, RADIUS, _lib.ptr(row_start),
                                                   _lib.ptr(ws), ws.numel(), s))
    count()
    K = int(row_start[total].item())
    corr = torch.empty((K, 2), dtype=torch.int32, device="cuda")
    table = torch.empty((Q, LIMIT), dtype=torch.int32, device="cuda")
    normals = torch.empty((Q, 3), dtype=torch.float64, device="cuda")
    variation = torch.empty((Q,), dtype=torch.float64, device="cuda")

    def fill():
        _lib.check(lib.prg_radius_fill_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), C, max_cloud, RADIUS, _lib.ptr(row_start), K,
                                                  _lib.ptr(corr), s))

    def select():
        _lib.check(lib.prg_radius_select_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), C, max_cloud, _lib.ptr(row_start), _lib.ptr(corr), K,
                                                    LIMIT, _lib.ptr(d_o), _lib.ptr(base), None, _lib.ptr(table), s))
    fill()
    select()
    rs = row_start.cpu().numpy()
    m = np.concatenate([np.diff(rs[b:b + n + 1]) for b, n in zip(offs.cpu().numpy()[0::2], sizes)])
    cnt = torch.from_numpy(m.astype(np.int32)).cuda()

    def kernel(var):
        def run():
            _lib.check(lib.prg_normals_ragged_f64(_lib.ptr(stack), _lib.ptr(d_o), C, _lib.ptr(table), _lib.ptr(d_o), None, _lib.ptr(cnt),
                                                  Q, LIMIT, _lib.ptr(views), 3, _lib.ptr(normals), _lib.ptr(variation) if var else None,
                                                  None, s))
        return run
    kernel(True)()
    want_n, want_v = PP.estimate_normals_cloud(clouds[0], RADIUS, LIMIT, viewpoint=views[0].cpu().numpy())
    n0 = len(clouds[0])
    if not (np.array_equal(normals[:n0].cpu().numpy().view(np.uint64), want_n.view(np.uint64)) and
            np.array_equal(variation[:n0].cpu().numpy().view(np.uint64), want_v.view(np.uint64))):
        raise SystemExit("the first cloud's normals differ from the numpy specification")
    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "clouds": C, "rows": Q, "rows_per_cloud_median": float(np.median(sizes)),
           "radius": RADIUS, "limit": LIMIT, "K": K, "matches_per_row_mean": float(m.mean()), "rows_truncated_share": float((m > LIMIT).mean()),
           "count": timed(count, a.repeats), "fill": timed(fill, a.repeats), "select": timed(select, a.repeats),
           "normals": timed(kernel(False), a.repeats), "normals_with_variation": timed(kernel(True), a.repeats)}
    res["search_ms"] = res["count"]["ms_median"] + res["fill"]["ms_median"] + res["select"]["ms_median"]
    # what the kernel must move at least: the table row, count, the row itself, the outputs; the gathered neighbours come from L2
    res["normals_min_bytes"] = int(Q * (4 * LIMIT + 4 + 24 + 24))
    res["normals_min_bytes_over_time_GBps"] = res["normals_min_bytes"] / (res["normals"]["ms_median"] * 1e-3) / 1e9
    lens = [int(n) for n in sizes]
    layer = []
    for _ in range(3 + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G.estimate_normals(stack, lens, radius=RADIUS, limit=LIMIT, viewpoints=views)
        torch.cuda.synchronize()
        layer.append(1e3 * (time.perf_counter() - t0))
    res["layer_ms"] = {"ms_median": statistics.median(layer[3:]), "ms_min": min(layer[3:]), "ms_max": max(layer[3:]), "repeats": a.repeats}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
