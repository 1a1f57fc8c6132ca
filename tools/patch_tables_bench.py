#!/usr/bin/env python
"""What the coarse-level ground truth costs on the device.  One GPU.  Writes profiles/patch_tables_bench.json.

Input: `--items` (16 and 250) items of two voxel-like clouds of ~4.5 k rows — tools/neighbor_tables_bench.py's clouds: a 2.5 cm
grid surface patch with a few millimetres of jitter, and the same patch moved by a centimetre of noise and permuted — with the
10 cm voxel means of each cloud as its nodes (~300 per cloud: the third level of a pyramid that starts at 2.5 cm).  limit 64,
radius 0.05.  Timed, each on preallocated buffers with HIP events around the call, median of `--repeats` (20) after 3 warm-up calls:

  nearest          prg_nearest_ragged_f64 on [points_c | nodes_c] per cloud (both directions: the call has no one-sided form)
  tables           prg_patch_tables_ragged (pad pass + rank pass) on its output
  overlap          prg_patch_overlap_ragged_f64 with the bounding-box pre-filter (box pass + hits pass)
  overlap_plain    the same call with boxes = NULL: every patch pair tested
  layers           geometry.node_patches_ragged + geometry.patch_overlaps_ragged end to end, allocations, nonzero, gather and the
                   one read-back included (HIP events around the two Python calls)

The first item's tables and overlaps are compared with the numpy specification before anything is timed.

    python tools/patch_tables_bench.py [--out profiles/patch_tables_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT, RADIUS, NODE_VOXEL = 64, 0.05, 0.1


def voxel_like_pair(rng, n):
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 0.025
    a = np.concatenate([g, 1.5 + 0.1 * np.sin(3 * g[:, :1])], 1) + rng.uniform(-0.004, 0.004, (n, 3))
    b = a + rng.normal(0, 0.01, (n, 3))
    return a[rng.permutation(n)], b[rng.permutation(n)]


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


def leg(n_items, rows, repeats):
    import torch

    from pointreggpt_amd import _lib
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    lib = _lib.load()
    rng = np.random.default_rng(n_items)
    clouds = [c for n in rng.integers(int(rows * 0.8), int(rows * 1.2) + 1, size=n_items) for c in voxel_like_pair(rng, int(n))]
    nodes = [PP.voxel_down_sample(c, NODE_VOXEL) for c in clouds]
    C = len(clouds)
    pn, nn = np.array([len(c) for c in clouds], dtype=np.int64), np.array([len(q) for q in nodes], dtype=np.int64)
    po, no = np.concatenate([[0], np.cumsum(pn)]), np.concatenate([[0], np.cumsum(nn)])
    d_points, d_nodes = torch.from_numpy(np.concatenate(clouds)).cuda(), torch.from_numpy(np.concatenate(nodes)).cuda()
    s = _lib.stream_ptr()
    dev = lambda a, t=np.int64: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda()       # noqa: E731

    # the specification on the first item, against the layers
    assign, table, sizes = G.node_patches_ragged(d_points, po, d_nodes, no, LIMIT)
    corr, hits, overlap, co = G.patch_overlaps_ragged(d_points, po, table, no, RADIUS)
    want = [PP.node_patches(clouds[c], nodes[c], LIMIT) for c in (0, 1)]
    for c in (0, 1):
        got = (assign[po[c]:po[c + 1]], table[no[c]:no[c + 1]], sizes[no[c]:no[c + 1]])
        if not all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want[c])):
            raise SystemExit("cloud {}'s patch tables differ from the numpy specification".format(c))
    w_corr, w_hits, w_ov = PP.patch_overlaps(clouds[0], want[0][1], clouds[1], want[1][1], RADIUS)
    k = int(co[1].item())
    if not (np.array_equal(corr[:k].cpu().numpy(), w_corr) and np.array_equal(hits[:k].cpu().numpy(), w_hits)
            and overlap[:k].cpu().numpy().tobytes() == w_ov.tobytes()):
        raise SystemExit("the first item's overlaps differ from the numpy specification")

    # the four calls on preallocated buffers
    seg = np.stack([pn, nn], 1).reshape(-1)
    pair_offs = dev(np.concatenate([[0], np.cumsum(seg)]))
    buf = torch.cat([t[o[c]:o[c + 1]] for c in range(C) for t, o in ((d_points, po), (d_nodes, no))], 0)
    d2 = torch.full((buf.shape[0],), float("inf"), dtype=torch.float64, device="cuda")
    idx = torch.full((buf.shape[0],), -1, dtype=torch.int32, device="cuda")
    max_cloud, max_nodes = int(pn.max()), int(nn.max())
    t_offs, p_offs = dev(no), dev(po)
    tab = torch.empty((int(no[-1]), LIMIT), dtype=torch.int32, device="cuda")
    siz = torch.empty((int(no[-1]),), dtype=torch.int32, device="cuda")
    per_item = nn[0::2] * nn[1::2]
    h_offs = dev(np.concatenate([[0], np.cumsum(per_item)]))
    total = int(per_item.sum())
    dense = torch.empty((total, 2), dtype=torch.int32, device="cuda")
    boxes = torch.empty((int(no[-1]), 6), dtype=torch.float64, device="cuda")

    def nearest():
        _lib.check(lib.prg_nearest_ragged_f64(_lib.ptr(buf), _lib.ptr(pair_offs), C, max(max_cloud, max_nodes), _lib.ptr(d2),
                                              _lib.ptr(idx), s))

    def tables():
        _lib.check(lib.prg_patch_tables_ragged(_lib.ptr(d2), _lib.ptr(idx), _lib.ptr(pair_offs), C, max_cloud, max_nodes, LIMIT,
                                               _lib.ptr(t_offs), None, None, _lib.ptr(tab), _lib.ptr(siz), s))

    def overlap_call(bx):
        _lib.check(lib.prg_patch_overlap_ragged_f64(_lib.ptr(d_points), _lib.ptr(p_offs), n_items, _lib.ptr(tab), _lib.ptr(t_offs),
                                                    max_nodes, LIMIT, RADIUS, _lib.ptr(h_offs), total, int(per_item.max()),
                                                    _lib.ptr(bx), _lib.ptr(dense), s))

    def layers():
        _, t, _ = G.node_patches_ragged(d_points, po, d_nodes, no, LIMIT)
        G.patch_overlaps_ragged(d_points, po, t, no, RADIUS)

    nearest()
    tables()
    if not torch.equal(tab, table):
        raise SystemExit("the preallocated call's tables differ from the layer's")
    out = {"items": n_items, "clouds": C, "fine_rows": int(pn.sum()), "rows_per_cloud_median": float(np.median(pn)),
           "nodes": int(nn.sum()), "nodes_per_cloud_median": float(np.median(nn)), "limit": LIMIT, "radius": RADIUS,
           "members_per_node_mean": float(pn.sum() / nn.sum()), "patches_truncated_share": float((siz > LIMIT).float().mean().item()),
           "node_pairs": total, "node_pairs_listed": int(corr.shape[0]), "dense_hits_bytes": total * 8,
           "point_tests_per_rank_sweep": int((pn * pn).sum())}
    out["nearest"], out["tables"] = timed(nearest, repeats), timed(tables, repeats)
    out["overlap"] = timed(lambda: overlap_call(boxes), repeats)
    with_boxes = dense.clone()
    out["overlap_plain"] = timed(lambda: overlap_call(None), repeats)
    if not torch.equal(with_boxes, dense):
        raise SystemExit("the hits with and without the pre-filter differ")
    out["node_pairs_tested_share"] = float((with_boxes[:, 0] > 0).float().mean().item())
    out["layers"] = timed(layers, repeats)
    out["device_ms"] = out["nearest"]["ms_median"] + out["tables"]["ms_median"] + out["overlap"]["ms_median"]
    out["prefilter_speedup"] = out["overlap_plain"]["ms_median"] / out["overlap"]["ms_median"]
    print(json.dumps(out), flush=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--items", type=int, nargs="+", default=[16, 250])
    p.add_argument("--rows", type=int, default=4500)
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_tables_bench.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("patch_tables_bench.py measures on the GPU: no HIP device visible")
    res = {"device": torch.cuda.get_device_name(0), "legs": []}
    for n in a.items:
        res["legs"].append(leg(n, a.rows, a.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
