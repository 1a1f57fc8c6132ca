#!/usr/bin/env python
"""What the fine-level ground truth costs on the device.  One GPU.  Writes profiles/fine_labels_bench.json.

Input: tools/patch_tables_bench.py's — `--items` (16 and 250) items of two voxel-like clouds of ~4.5 k rows with the 10 cm voxel
means of each cloud as its nodes — as a two-level pyramid; `geometry.coarse_ground_truth` at limit 64, radius 0.05 gives the
listed node pairs, `geometry.select_node_corr` with min_overlap 0.1 and num_targets 128 under fixed keys the selected ones.
Timed, with HIP events around the call, median of `--repeats` (20) after 3 warm-up calls:

  kernel             prg_patch_corr_labels_f64 on preallocated buffers (the selected pairs, the label buffer)
  fine_ground_truth  geometry.fine_ground_truth end to end: the selection with its sorts and its one read-back, the gathers,
                     the allocation of the labels, the kernel
  torch              the same labels without the kernel: a gather of the patches' points and broadcast float64 arithmetic on the
                     device, dx*dx + dy*dy + dz*dz < r*r written out, then the slack row and column — the formulation the
                     kernel replaces; compared with the kernel's bytes before it is timed

The first item's labels are compared bit for bit with the numpy specification before anything is timed.

    python tools/fine_labels_bench.py [--out profiles/fine_labels_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT, RADIUS, NODE_VOXEL, MIN_OVERLAP, NUM_TARGETS = 64, 0.05, 0.1, 0.1, 128


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


def torch_labels(points, table, pairs, radius):
    """`postprocess.patch_corr_labels` in torch on the device: the same float64 expression, no kernel of this project's."""
    import torch
    n, K = points.shape[0], table.shape[1]
    valid = (table >= 0) & (table < n)
    pp = torch.cat([points, torch.full((1, 3), float("nan"), dtype=points.dtype, device=points.device)])[
        torch.where(valid, table, torch.full_like(table, n)).to(torch.int64)]                       # (M, K, 3), NaN in the pads
    a, b = pairs[:, 0].to(torch.int64), pairs[:, 1].to(torch.int64)
    A, B = pp[a][:, :, None, :], pp[b][:, None, :, :]
    dx, dy, dz = B[..., 0] - A[..., 0], B[..., 1] - A[..., 1], B[..., 2] - A[..., 2]
    w = dx * dx + dy * dy + dz * dz < radius * radius
    labels = torch.zeros((pairs.shape[0], K + 1, K + 1), dtype=torch.bool, device=points.device)
    labels[:, :K, :K] = w
    labels[:, :K, K] = valid[a] & ~w.any(2)
    labels[:, K, :K] = valid[b] & ~w.any(1)
    return labels


def leg(n_items, rows, repeats):
    import torch

    from pointreggpt_amd import _lib
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    lib = _lib.load()
    rng = np.random.default_rng(n_items)
    clouds = [c for n in rng.integers(int(rows * 0.8), int(rows * 1.2) + 1, size=n_items) for c in voxel_like_pair(rng, int(n))]
    nodes = [PP.voxel_down_sample(c, NODE_VOXEL) for c in clouds]
    pn, nn = np.array([len(c) for c in clouds], dtype=np.int64), np.array([len(q) for q in nodes], dtype=np.int64)
    no = np.concatenate([[0], np.cumsum(nn)])
    fine = np.concatenate(clouds)
    pyr = {"points": [torch.from_numpy(fine).cuda(), torch.from_numpy(np.concatenate(nodes)).cuda()],
           "lengths": [torch.from_numpy(pn).cuda(), torch.from_numpy(nn).cuda()]}
    gt = G.coarse_ground_truth(pyr, fine_level=0, limit=LIMIT, radius=RADIUS)
    P = int(gt["overlap"].shape[0])
    keys = torch.from_numpy(np.random.default_rng(7).random(P)).cuda()
    kw = dict(fine_level=0, radius=RADIUS, min_overlap=MIN_OVERLAP, num_targets=NUM_TARGETS)
    out = G.fine_ground_truth(pyr, gt, keys=keys, **kw)
    labels, pairs, so = out["labels"], out["node_corr"].contiguous(), out["sel_offsets"].cpu().numpy()
    S = int(pairs.shape[0])

    # the specification on the first item (its nodes are the first rows of the table; the pad stays out of range)
    k = int(so[1])
    want = PP.patch_corr_labels(fine, gt["table"][:int(no[2])].cpu().numpy(), pairs[:k].cpu().numpy(), RADIUS)
    if not np.array_equal(labels[:k].cpu().numpy(), want):
        raise SystemExit("the first item's labels differ from the numpy specification")

    points, table = pyr["points"][0], gt["table"].contiguous()
    buf = torch.empty((S, LIMIT + 1, LIMIT + 1), dtype=torch.uint8, device="cuda")
    s = _lib.stream_ptr()

    def kernel():
        _lib.check(lib.prg_patch_corr_labels_f64(_lib.ptr(points), points.shape[0], _lib.ptr(table), table.shape[0], LIMIT,
                                                 _lib.ptr(pairs), S, RADIUS, _lib.ptr(buf), s))

    kernel()
    if not torch.equal(buf.view(torch.bool), labels):
        raise SystemExit("the preallocated call's labels differ from the layer's")
    if not torch.equal(torch_labels(points, table, pairs, RADIUS), labels):
        raise SystemExit("the torch formulation's labels differ from the kernel's")
    nbytes = S * (LIMIT + 1) ** 2
    patch = labels[:, :LIMIT, :LIMIT]
    res = {"items": n_items, "fine_rows": int(pn.sum()), "nodes": int(nn.sum()), "limit": LIMIT, "radius": RADIUS,
           "min_overlap": MIN_OVERLAP, "num_targets": NUM_TARGETS, "node_pairs_listed": P,
           "candidates": int((gt["overlap"] > MIN_OVERLAP).sum().item()), "selected": S, "labels_bytes": nbytes,
           "labels_true_share": float(patch.float().mean().item()),
           "valid_slots_share": float(out["src_mask"].float().mean().item()),
           "torch_temporary_bytes_each": S * LIMIT * LIMIT * 8}
    res["kernel"] = timed(kernel, repeats)
    res["fine_ground_truth"] = timed(lambda: G.fine_ground_truth(pyr, gt, keys=keys, **kw), repeats)
    res["select_node_corr"] = timed(lambda: G.select_node_corr(gt, min_overlap=MIN_OVERLAP, num_targets=NUM_TARGETS, keys=keys),
                                    repeats)
    res["torch"] = timed(lambda: torch_labels(points, table, pairs, RADIUS), repeats)
    res["kernel_write_GBps"] = nbytes / res["kernel"]["ms_median"] / 1e6
    res["torch_over_kernel"] = res["torch"]["ms_median"] / res["kernel"]["ms_median"]
    print(json.dumps(res), flush=True)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--items", type=int, nargs="+", default=[16, 250])
    p.add_argument("--rows", type=int, default=4500)
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_labels_bench.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fine_labels_bench.py measures on the GPU: no HIP device visible")
    res = {"device": torch.cuda.get_device_name(0), "legs": []}
    for n in a.items:
        res["legs"].append(leg(n, a.rows, a.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
