#!/usr/bin/env python
"""What writing gt.log while generating costs and saves.  One GPU.  Writes profiles/gt_at_generation.json.

(a) `--kernel`: prg_rigid_crop_ragged_f64 alone at 2 M and 20 M rows in 64 equal segments, every segment moved, crop box on, no
    input mask (24 B in, 24 B + 1 B out per row), out of place; HIP events around the one launch, median of `--repeats` (20)
    after warm-up, GB/s = 49 B x rows / time.  Before every timed launch a 1 GiB fill is queued: while the GPU works on it the
    host gets ahead, so the interval between the events holds the kernel and not the host's time to issue it, and the input
    is not left in the 256 MiB Infinity Cache.  The output is compared bit for bit with the numpy specification on a slice first.
(b) `--wall --parent DIR`: wall seconds of whole processes on identical arguments (bf16, dim 64, 128x128, batch 64, the
    1000-step sampler, 256 synthetic scenes), alternated, `--wall-repeats` (3) each after one warm-up pair:
        two passes  = DIR/generate_dataset.py            then DIR/generate_gt.py    (DIR: a built checkout of the parent commit)
        one pass    = generate_dataset.py --with_gt      then generate_gt.py        (this tree; the second is the gather only)
    Every process is fresh (the page cache, the code-object cache and the allocator start as they would for a user), runs
    under its own time limit, and the first one that fails ends the measurement.  The two metadata/gt.log must be equal.

    python tools/gt_at_generation_bench.py --kernel --wall --parent ../parent [--out profiles/gt_at_generation.json]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_leg(repeats):
    import torch

    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    rng = np.random.default_rng(0)
    B = 64
    T = np.stack([np.eye(4)] * B)
    for b in range(B):
        a = rng.uniform(-0.3, 0.3)
        T[b, :3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
        T[b, :3, 3] = rng.uniform(-0.4, 0.4, 3)
    rows_out = []
    for total in (2_000_000, 20_000_000):
        per = total // B
        pts = torch.rand((total, 3), dtype=torch.float64, device="cuda") * 4.0 - torch.tensor([2.0, 2.0, 0.0], dtype=torch.float64,
                                                                                             device="cuda")
        offs = torch.arange(B + 1, dtype=torch.int64, device="cuda") * per
        out, vout = torch.empty_like(pts), torch.empty((total,), dtype=torch.uint8, device="cuda")
        box = (PP.BBOX_MIN, PP.BBOX_MAX)
        for _ in range(5):
            G.rigid_crop_ragged(pts, None, offs, T=T, crop=box, out=out, valid_out=vout)
        torch.cuda.synchronize()
        b = B - 1                                        # the last segment against the specification, bit for bit
        seg = pts[b * per:(b + 1) * per].cpu().numpy()
        want = PP.rigid_move(seg, T[b])
        keep = np.all((want >= box[0]) & (want <= box[1]), axis=1)
        if out[b * per:(b + 1) * per].cpu().numpy().tobytes() != want.tobytes() or \
                not np.array_equal(vout[b * per:(b + 1) * per].cpu().numpy() != 0, keep):
            raise SystemExit("prg_rigid_crop_ragged_f64 differs from the numpy specification")
        Td = torch.from_numpy(T).cuda()                  # the matrices uploaded once: only the launch is timed
        spacer = torch.empty((1 << 30,), dtype=torch.uint8, device="cuda")
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            spacer.zero_()
            e0.record()
            G.rigid_crop_ragged(pts, None, offs, T=Td, crop=box, out=out, valid_out=vout)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        r = {"rows": total, "segments": B, "bytes_per_row": 49, "ms_median": med, "ms_min": min(ms), "repeats": repeats,
             "GBps_median": 49.0 * total / (med * 1e-3) / 1e9, "GBps_best": 49.0 * total / (min(ms) * 1e-3) / 1e9,
             "kept_fraction": float((vout != 0).float().mean().item()), "bit_identical_to_specification": True}
        print(json.dumps(r), flush=True)
        rows_out.append(r)
        del pts, out, vout, spacer
    return {"what": "prg_rigid_crop_ragged_f64: every segment moved, crop on, no input mask, out of place; HIP events around the "
                    "launch behind a 1 GiB fill (host ahead of the GPU, input not cache-resident), median after 5 warm-up launches; next to it: prg_unproject_f64, the comparable streaming kernel, "
                    "3.9 TB/s (DESIGN.md §4.4)", "shapes": rows_out}


def run(cmd, cwd, root, limit):
    env = dict(os.environ, PYTHONPATH=root)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=limit)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("{} failed ({}) after {:.1f} s; nothing more is started:\n{}".format(
            " ".join(cmd), r.returncode, dt, r.stderr[-3000:]))
    return dt


def wall_leg(a):
    parent = os.path.abspath(a.parent)
    for root in (parent, ROOT):
        if not os.path.exists(os.path.join(root, "pointreggpt_amd", "libprg_hip.so")):
            raise SystemExit(f"{root}: libprg_hip.so is not built")
    common = ["--dataset_name", "ds", "-start", "0", "-stop", str(a.scenes)]
    gen = ["--resume", "synthetic:1", "--synthetic", "0", "--image_size", str(a.size), "--timesteps", "1000", "--sampling_timesteps",
           str(a.sampling_steps), "--batch_size", str(a.batch), "--dim", "64", "--dtype", "bf16"] + common
    arms = {"two_pass": (parent, []), "one_pass": (ROOT, ["--with_gt"])}
    walls = {k: {"generate_dataset_s": [], "generate_gt_s": [], "total_s": []} for k in arms}
    logs = {}
    tmp = tempfile.mkdtemp(prefix="gt_at_generation_", dir=a.workdir)
    try:
        for rep in range(-1, a.wall_repeats):              # rep -1: one warm-up pair, not reported
            for arm, (root, extra) in arms.items():
                cwd = os.path.join(tmp, f"{arm}{rep}")
                os.makedirs(cwd)
                t_gen = run([sys.executable, os.path.join(root, "generate_dataset.py")] + gen + extra, cwd, root, a.limit)
                t_gt = run([sys.executable, os.path.join(root, "generate_gt.py"), "--disable_tqdm"] + common, cwd, root, a.limit)
                with open(os.path.join(cwd, "ds", "metadata", "gt.log"), "rb") as f:
                    logs[arm] = f.read()
                shutil.rmtree(cwd)
                print(json.dumps({"rep": rep, "arm": arm, "generate_dataset_s": t_gen, "generate_gt_s": t_gt}), flush=True)
                if rep >= 0:
                    w = walls[arm]
                    w["generate_dataset_s"].append(t_gen), w["generate_gt_s"].append(t_gt), w["total_s"].append(t_gen + t_gt)
            if logs["one_pass"] != logs["two_pass"]:
                raise SystemExit("metadata/gt.log differs between the two arms")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for w in walls.values():
        for k in list(w):
            w[k + "_median"] = statistics.median(w[k])
    two, one = walls["two_pass"], walls["one_pass"]
    spread = max(two["total_s"]) - min(two["total_s"])
    return {"what": f"wall seconds of fresh processes, alternated after one warm-up pair: {a.scenes} synthetic scenes, {a.size}x{a.size}, "
                    f"dim-64 bf16 synthetic weights, batch {a.batch}, sampling_timesteps {a.sampling_steps} of 1000, the CLI's default "
                    "two lanes; two_pass = the parent commit's generate_dataset.py + generate_gt.py, one_pass = generate_dataset.py "
                    "--with_gt + generate_gt.py (gather only)",
            "two_pass": two, "one_pass": one, "gt_log_lines": len(logs["two_pass"].splitlines()), "gt_log_identical": True,
            "one_pass_minus_two_pass_total_s": one["total_s_median"] - two["total_s_median"],
            "generate_dataset_leg_added_s": one["generate_dataset_s_median"] - two["generate_dataset_s_median"],
            "two_pass_total_spread_s": spread,
            "one_pass_within_two_pass_plus_spread": one["total_s_median"] <= two["total_s_median"] + spread}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kernel", action="store_true")
    p.add_argument("--wall", action="store_true")
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit (for --wall)")
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--wall-repeats", type=int, default=3)
    p.add_argument("--scenes", type=int, default=256)
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--sampling-steps", type=int, default=1000)
    p.add_argument("--limit", type=int, default=300, help="time limit of one process, seconds")
    p.add_argument("--workdir", default=None, help="where the datasets are written (default: the system's temporary folder)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_at_generation.json"))
    a = p.parse_args()
    if not (a.kernel or a.wall):
        p.error("nothing to do: --kernel and / or --wall")
    if a.wall and not a.parent:
        p.error("--wall needs --parent")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gt_at_generation_bench.py measures on the GPU: no HIP device visible")
    res = {"device": torch.cuda.get_device_name(0), "host_cpus_usable": len(os.sched_getaffinity(0))}
    if os.path.exists(a.out):                              # the two legs may be measured in separate runs
        with open(a.out) as f:
            res.update({k: v for k, v in json.load(f).items() if k in ("kernel", "wall")})
    if a.wall:                                             # first: this process has not touched the GPU's memory yet
        res["wall"] = wall_leg(a)
        print(json.dumps(res["wall"]), flush=True)
    if a.kernel:
        res["kernel"] = kernel_leg(a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
