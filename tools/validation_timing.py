#!/usr/bin/env python
"""Time the forward process and the loss of the validation path (prg_q_sample + prg_diffusion_loss, csrc/validate.hip) next to
the same arithmetic written in torch on the same device.  Information only: there is no speed gate on these kernels.

    python tools/validation_timing.py [--out profiles/validation_timing.json]

Shapes: B = 64 at 128x128 and 256x256 (the workload's), and the 16 Mpx streaming point (B = 1, HW = 2^24) quoted for the other
memory-bound kernels.  Per shape and noise source (stored, Philox) and implementation: `rounds` windows of `reps` back-to-back
calls between two device events after a warm-up of the shape, the two implementations alternating window by window; median and
spread of the per-call time, and the algorithmic bytes per call over it.  Algorithmic bytes (each element once):
q_sample reads x0 (+ noise) and writes x_t; the pred_v L1 loss reads u, x0 (+ noise): 4 B per element each.  Needs a HIP device:
without one it fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_pair(u, x0, n, a, s, w):
    """q_sample and the pred_v L1 loss as torch writes them (sd:1451-1453, 1164-1167, 1493-1497), on the device."""
    x_t = a[:, None] * x0 + s[:, None] * n
    v = a[:, None] * n - s[:, None] * x0
    mean = (u - v).abs().mean(dim=1)
    return x_t, torch.stack([mean, mean * w], dim=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_timing.json"))
    p.add_argument("--reps", default=50, type=int)
    p.add_argument("--rounds", default=7, type=int)
    args = p.parse_args()
    from pointreggpt_amd import _lib, validate as V
    _lib.require_gpu()
    name = torch.cuda.get_device_name(0)
    results = []
    for label, B, HW in (("128x128, B = 64", 64, 128 * 128), ("256x256, B = 64", 64, 256 * 256), ("16 Mpx, B = 1", 1, 1 << 24)):
        g = torch.Generator(device="cuda").manual_seed(B + HW)
        x0, n, u = (torch.randn((B, HW), device="cuda", generator=g) for _ in range(3))
        a = torch.full((B,), 0.6, device="cuda")
        s = torch.full((B,), 0.8, device="cuda")
        w = torch.ones((B,), device="cuda")
        seeds = list(range(B))

        def hip_stored():
            V.q_sample_hip(x0, a, s, n)
            V.diffusion_loss_hip(u, x0, a, s, w, 2, 0, n)

        def hip_philox():
            V.q_sample_hip(x0, a, s, seeds=seeds)
            V.diffusion_loss_hip(u, x0, a, s, w, 2, 0, seeds=seeds)

        def in_torch():
            torch_pair(u, x0, n, a, s, w)

        impls = {"hip_stored": hip_stored, "hip_philox": hip_philox, "torch_stored": in_torch}
        # same results before any timing (the torch sum's order differs: last bits)
        x_t, tab = torch_pair(u, x0, n, a, s, w)
        same_x_t = bool(torch.equal(V.q_sample_hip(x0, a, s, n), x_t))
        got = V.diffusion_loss_hip(u, x0, a, s, w, 2, 0, n)
        loss_gap = float(((got[:, 0] - tab[:, 0].double()).abs() / got[:, 0]).max())
        for f in impls.values():                              # warm-up of this shape
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in impls}
        for _ in range(args.rounds):
            for k, f in impls.items():                        # alternating, window by window
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.reps)
        elems = B * HW
        nbytes = {"hip_stored": 4 * elems * 6, "hip_philox": 4 * elems * 4, "torch_stored": 4 * elems * 6}
        row = {"shape": label, "B": B, "HW": HW, "x_t_equals_torch_bitwise": same_x_t, "loss_relative_gap_to_torch_float32": loss_gap}
        for k, v in times.items():
            med = statistics.median(v)
            row[k] = {"us_per_call_median": med, "us_min": min(v), "us_max": max(v), "algorithmic_bytes": nbytes[k],
                      "algorithmic_TB_per_s": nbytes[k] / (med * 1e-6) / 1e12}
        results.append(row)
        print(label, {k: f"{row[k]['us_per_call_median']:.1f} us ({row[k]['algorithmic_TB_per_s']:.2f} TB/s)" for k in times})
    out = {"device": name, "reps": args.reps, "rounds": args.rounds,
           "method": "device events around `reps` back-to-back calls (q_sample + pred_v L1 loss, host wrappers included), "
                     "`rounds` windows per implementation alternating, median [min, max]; algorithmic bytes = each element once",
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
