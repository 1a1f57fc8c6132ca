#!/usr/bin/env python
"""Device voxel grid (prg_voxel_grid_ragged) against the host grid (prg_host_voxel_down_sample, one cloud at a time on the
calling thread) on identical inputs, and the multi-sample generator end to end with either backend.

One process, one GPU.  Device times are HIP events around the whole call (all of its launches) after warm-up, median and
minimum of `--repeats`; host times are time.perf_counter around the serial per-cloud loop the callers run (the host code is
the same in either backend).  Outputs are compared bit for bit before anything is reported.  The end-to-end leg runs
Generator.generate(0, B, 3) with voxel_backend "host" and "device" alternately (same process, same networks, files written
to a temporary folder) and reports every wall time.  Writes profiles/voxel_grid_device.json.

    python tools/voxel_grid_bench.py [--repeats 20] [--e2e-scenes 64] [--e2e-size 128] [--e2e-sampling-steps N] [--no-e2e]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pointreggpt_amd import geometry as G  # noqa: E402
from pointreggpt_amd import postprocess as PP  # noqa: E402


def surface(rng, n, f32=False):
    """n points of a depth-map-like surface inside the crop box (x, y uniform, z a smooth sheet + 1 mm noise)."""
    x, y = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n)
    z = 2.0 + 0.3 * np.sin(2.0 * x) * np.cos(1.5 * y) + 0.001 * rng.standard_normal(n)
    p = np.stack([x, y, z], 1)
    return p.astype(np.float32).astype(np.float64) if f32 else p


def shapes(rng):
    yield ("memory update B=64 128x128 (16k memory + 16k new rows per scene)", 0.002,
           [np.concatenate([surface(rng, 16384, True), surface(rng, 16384)]) for _ in range(64)])
    yield ("third view B=16 256x256 (130k memory + 65k new rows per scene)", 0.002,
           [np.concatenate([surface(rng, 130000, True), surface(rng, 65536)]) for _ in range(16)])
    yield ("generate_gt launch: 1024 clouds of ~20k rows", 0.025,
           [surface(rng, int(n)) for n in rng.integers(18000, 22000, 1024)])


def time_shape(name, v, segs, repeats, host_repeats):
    offs = np.zeros(len(segs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in segs])
    pts = torch.from_numpy(np.concatenate(segs, 0)).cuda()
    d_offs = torch.from_numpy(offs).cuda()
    for _ in range(3):
        out, oo, st = G.voxel_grid_ragged(pts, None, d_offs, v)
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, oo, st = G.voxel_grid_ragged(pts, None, d_offs, v)
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    host_ms, host_out = [], None
    for _ in range(host_repeats):
        t0 = time.perf_counter()
        host_out = [PP.native_voxel_down_sample(s, v) for s in segs]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    out, oo, st = out.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()
    if st.any():
        raise SystemExit(f"{name}: status {st[st != 0]}")
    for b, h in enumerate(host_out):
        if out[oo[b]:oo[b + 1]].tobytes() != h.tobytes():
            raise SystemExit(f"{name}: segment {b} differs from the host grid")
    return {"shape": name, "segments": len(segs), "rows_in": int(offs[-1]), "rows_out": int(oo[-1]), "voxel": v,
            "device_ms_median": statistics.median(dev_ms), "device_ms_min": min(dev_ms), "device_repeats": repeats,
            "host_serial_ms_median": statistics.median(host_ms), "host_serial_ms_min": min(host_ms),
            "host_repeats": host_repeats, "bit_identical": True}


def end_to_end(a):
    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.generator import Generator
    from pointreggpt_amd.unet import MaskUnet, Unet
    S, B = a.e2e_size, a.e2e_scenes
    unet = Unet(64, dtype="bf16").init_synthetic(seed=1, calibrated=True)
    mask = MaskUnet(64, dtype="bf16").init_synthetic(seed=2, calibrated=True)
    diff = GaussianDiffusion(unet, image_size=S, timesteps=1000, sampling_timesteps=a.e2e_sampling_steps)
    walls = {"host": [], "device": []}
    with tempfile.TemporaryDirectory() as tmp:
        run = 0

        def once(backend):
            nonlocal run
            run += 1
            gen = Generator(diff, None, batch_size=B, samples_folder=os.path.join(tmp, f"r{run}", "data"), synthetic_seed=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gen.generate(0, B, 3, depth_correction=mask, noise_seed=0, voxel_backend=backend)   # returns when all files exist
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        once("device"), once("host")                       # warm-up of both (code objects, graphs, allocator, page cache)
        for _ in range(a.e2e_repeats):
            for backend in ("host", "device"):
                walls[backend].append(once(backend))
    diff.close(); unet.close(); mask.close()
    chain = "1000-step ancestral DDNM (the shipped sampler)" if a.e2e_sampling_steps is None else f"{a.e2e_sampling_steps}-step DDIM"
    return {"what": f"wall seconds of Generator.generate(0, {B}, 3) at {S}x{S}, dim-64 bf16 calibrated synthetic weights, one lane, "
                    f"{chain}, files written; backends alternated in one process after one warm-up run each",
            "host_backend_s": walls["host"], "device_backend_s": walls["device"],
            "host_backend_s_median": statistics.median(walls["host"]),
            "device_backend_s_median": statistics.median(walls["device"])}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--host-repeats", type=int, default=3)
    p.add_argument("--e2e-scenes", type=int, default=64)
    p.add_argument("--e2e-size", type=int, default=128)
    p.add_argument("--e2e-sampling-steps", type=int, default=None)
    p.add_argument("--e2e-repeats", type=int, default=3)
    p.add_argument("--no-e2e", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_grid_device.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_grid_bench.py measures on the GPU: no HIP device visible")
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "host_cpus_usable": len(os.sched_getaffinity(0)), "grid": []}
    for name, v, segs in shapes(rng):
        r = time_shape(name, v, segs, a.repeats, a.host_repeats)
        print(json.dumps(r), flush=True)
        res["grid"].append(r)
    if not a.no_e2e:
        res["end_to_end"] = end_to_end(a)
        print(json.dumps(res["end_to_end"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
