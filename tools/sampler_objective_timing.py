"""Time sampler_step_kernel alone per objective: HIP-event microseconds per launch of prg_debug_sampler_step_objective at
(B, HW) = (64, 16384) for objectives 0, 1, 2, and, with --parent-lib, of prg_debug_sampler_step_keep in a library built from the
parent commit (the same kernel before the objectives existed).  The variants alternate within one process, `--rounds` times, so that
the run-to-run spread of each is seen next to the differences between them.

    python tools/sampler_objective_timing.py [--parent-lib /path/to/parent/libprg_hip.so] [--rounds 9] [--reps 400]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointreggpt_amd import _lib  # noqa: E402
from pointreggpt_amd.diffusion import GaussianDiffusion  # noqa: E402


class _Net:
    channels = out_dim = 1
    random_or_learned_sinusoidal_cond = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", default=9, type=int)
    ap.add_argument("--reps", default=400, type=int)
    ap.add_argument("--batch", default=64, type=int)
    ap.add_argument("--pixels", default=16384, type=int)
    args = ap.parse_args()
    B, HW = args.batch, args.pixels
    lib = _lib.load()
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        parent.prg_debug_sampler_step_keep.restype, parent.prg_debug_sampler_step_keep.argtypes = _lib.PROTOTYPES["prg_debug_sampler_step_keep"]
        assert not hasattr(parent, "prg_sampler_set_objective"), "--parent-lib already has the objectives"
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn((B, HW), generator=g).cuda()
    u = (torch.rand((B, HW), generator=g) * 4 - 2).cuda()
    cond = torch.cat([torch.rand((B, 1, HW), generator=g) * 2 - 1, (torch.rand((B, 1, HW), generator=g) > 0.45).float() * 2 - 1], 1).cuda()
    seeds = torch.arange(B, dtype=torch.int64).cuda()
    tables = {}
    for name, code in (("pred_x0", 0), ("pred_noise", 1), ("pred_v", 2)):
        d = GaussianDiffusion(_Net(), image_size=128, timesteps=1000, sampling_timesteps=20, objective=name, beta_schedule="sigmoid")
        r = d.step_table()[10]                                   # a DDIM row with eps and noise: what a production run mostly launches
        p, q = (d.objective_table() or [(0.0, 0.0)] * 20)[10]
        tables[code] = (_lib.StepC(r["t"], r["clip_pred"], r["c_x0"], r["c_x"], r["c_eps"], r["sigma"], r["sqrt_recip"], r["sqrt_recipm1"]), p, q)

    def timed(which):
        x = x0.clone()
        us = C.c_float()
        if which == "parent":
            rc = parent.prg_debug_sampler_step_keep(_lib.ptr(x), _lib.ptr(u), _lib.ptr(cond), _lib.ptr(seeds), C.byref(tables[0][0]), -1.0, None,
                                                    B, HW, args.reps, C.byref(us), None)
            assert rc == 0, rc
        else:
            row, p, q = tables[which]
            _lib.check(lib.prg_debug_sampler_step_objective(_lib.ptr(x), _lib.ptr(u), _lib.ptr(cond), _lib.ptr(seeds), C.byref(row), which, p, q,
                                                            -1.0, None, B, HW, args.reps, C.byref(us), None))
        return us.value

    variants = (["parent"] if parent is not None else []) + [0, 1, 2]
    for v in variants:
        timed(v)                                                 # warm-up: code objects, first touch
    got = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:
            got[v].append(timed(v))
    label = {"parent": "parent commit, prg_debug_sampler_step_keep", 0: "objective 0 (pred_x0)", 1: "objective 1 (pred_noise)",
             2: "objective 2 (pred_v)"}
    print(f"sampler_step_kernel alone, (B, HW) = ({B}, {HW}), {args.reps} launches per measurement, {args.rounds} alternating rounds, "
          f"{torch.cuda.get_device_name(0)}")
    for v in variants:
        a = np.array(got[v])
        print(f"  {label[v]:48s} median {np.median(a):7.2f} us   min {a.min():7.2f}   max {a.max():7.2f}   spread (max - min) {a.max() - a.min():5.2f}")


if __name__ == "__main__":
    main()
