#!/usr/bin/env python
"""Is a dataset generated in a fast arithmetic mode the same dataset, only faster?    One GPU.  Writes
profiles/dataset_equivalence.json.

The same 256 synthetic scenes (one synthetic seed, one noise seed: a scene's poses and noise do not depend on dtype, batch or
lane) are generated through `Generator.generate(gt_log=True)` with the weights of bench.py's pipeline leg
(`init_synthetic(seed=1 / 2, calibrated=True)`, dim 64), 128x128, the 1000-step chain, B = 64, once each in fp32, f16x3, bf16
and mxfp8, plus a control: fp32 again on two lanes, which must compare as identical.  Every other dataset is then compared
with the first fp32 one by `pointreggpt_amd.compare.compare_datasets` (nearest-neighbour distances between the clouds in
both directions, gt.log line by line).  Last, the nearest-neighbour launch itself is timed on the fp32 / bf16 clouds of all
256 scenes: HIP events around the one prg_nearest_ragged_f64 call, median of `--repeats` after warm-up, and the candidate
evaluations (2 * rows of a * rows of b, summed over the cloud pairs) per second that implies.  No pass mark is set for any
number here: they are written down.

    python tools/dataset_equivalence.py run [--workdir DIR] [--out profiles/dataset_equivalence.json]

`run` starts one fresh process per dataset and per comparison (the sub-commands below), each under `timeout -k 10 LIMIT`
with LIMIT = 2 x scenes / the README's pairs/s of the mode + 90 s for start-up and graph capture, one after the other, and
starts nothing more after the first one that fails.  The datasets are deleted at the end; the report keeps the summaries.

    python tools/dataset_equivalence.py generate --dtype bf16 --out DIR [--lanes 2]
    python tools/dataset_equivalence.py compare A B --out piece.json
    python tools/dataset_equivalence.py kernel A B --out piece.json
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

README_PAIRS_PER_S = {"fp32": 1.21, "f16x3": 5.0, "bf16": 14.4, "mxfp8": 14.4}     # mxfp8: the README rates it at 1.07 x bf16
STARTUP_S = 90
# nearest_ragged_kernel as `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage` reports it for csrc/geometry.hip
KERNEL_RESOURCES = {"vgprs": 83, "agprs": 0, "sgprs": 30, "scratch_bytes_per_lane": 0, "lds_bytes_per_workgroup": 6144,
                    "waves_per_simd": 5, "threads_per_workgroup": 256, "queries_per_thread": 2, "tile_rows": 256}


def generate(a):
    import torch

    from pointreggpt_amd.diffusion import GaussianDiffusion
    from pointreggpt_amd.generator import Generator, gather_gt
    from pointreggpt_amd.unet import MaskUnet, Unet
    if not torch.cuda.is_available():
        raise SystemExit("dataset_equivalence.py generates on the GPU: no HIP device visible")

    def lane():
        unet = Unet(a.dim, dtype=a.dtype).init_synthetic(seed=1, calibrated=True)
        mask = MaskUnet(a.dim, dtype=a.dtype).init_synthetic(seed=2, calibrated=True)
        return GaussianDiffusion(unet, image_size=a.size, timesteps=1000, sampling_timesteps=a.sampling_steps), mask

    out = os.path.abspath(a.out)
    (diff, mask), lanes = lane(), [lane() for _ in range(1, a.lanes)]
    gen = Generator(diff, None, batch_size=a.batch, samples_folder=os.path.join(out, "data"), synthetic_seed=a.seed)
    stats = {}
    t0 = time.perf_counter()
    gen.generate(0, a.scenes, 1, depth_correction=mask, noise_seed=a.noise_seed, gt_log=True, lanes=lanes, stats=stats)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gather_gt(os.path.basename(out), 0, a.scenes, root=os.path.dirname(out))
    info = {"dtype": a.dtype, "scenes": a.scenes, "batch": a.batch, "lanes": stats.get("lanes", a.lanes), "size": a.size,
            "sampling_steps": a.sampling_steps, "dim": a.dim, "synthetic_seed": a.seed, "noise_seed": a.noise_seed,
            "generate_s": dt, "pairs_per_s_including_warm_up": a.scenes / dt}
    with open(os.path.join(out, "generated.json"), "w") as f:
        json.dump(info, f)
    print(json.dumps(info), flush=True)


def compare(a):
    from pointreggpt_amd.compare import compare_datasets
    t0 = time.perf_counter()
    rep = compare_datasets(a.a, a.b, 0, a.scenes, scenes_per_launch=a.scenes)
    piece = {"summary": rep["summary"], "gt_lines": rep["gt"]["lines"], "compare_s": time.perf_counter() - t0,
             "rows_a": sum(e.get("n_a", 0) for e in rep["clouds"]), "rows_b": sum(e.get("n_b", 0) for e in rep["clouds"])}
    for side, root in (("a", a.a), ("b", a.b)):
        with open(os.path.join(root, "generated.json")) as f:
            piece[side] = json.load(f)
    with open(a.out, "w") as f:
        json.dump(piece, f)
    print(json.dumps(piece["summary"]), flush=True)


def kernel(a):
    import numpy as np
    import torch

    from pointreggpt_amd import _lib
    from pointreggpt_amd import geometry as G
    from pointreggpt_amd import postprocess as PP
    from pointreggpt_amd.compare import _cloud_path
    from pathlib import Path
    lib = _lib.load()
    _lib.require_gpu()
    pairs = [(PP.read_ply(str(_cloud_path(Path(a.a), i, k))), PP.read_ply(str(_cloud_path(Path(a.b), i, k))))
             for i in range(a.scenes) for k in (0, 1)]
    clouds = [c for p in pairs for c in p]
    sizes = np.array([len(c) for c in clouds], dtype=np.int64)
    evaluations = int(sum(2 * len(x) * len(y) for x, y in pairs))
    pts, offs = G.upload_clouds(clouds, "cuda", dtype=np.float64)
    d2 = torch.empty((pts.shape[0],), dtype=torch.float64, device="cuda")
    idx = torch.empty((pts.shape[0],), dtype=torch.int32, device="cuda")

    def launch():
        _lib.check(lib.prg_nearest_ragged_f64(_lib.ptr(pts), _lib.ptr(offs), len(pairs), int(sizes.max()), _lib.ptr(d2),
                                              _lib.ptr(idx), _lib.stream_ptr()), "prg_nearest_ragged_f64")

    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    want_d2, want_idx = PP.nearest(pairs[-1][1], pairs[-1][0])       # the last cloud against the specification, bit for bit
    lo = int(offs[-2].item())
    if d2[lo:].cpu().numpy().tobytes() != want_d2.tobytes() or not np.array_equal(idx[lo:].cpu().numpy(), want_idx):
        raise SystemExit("prg_nearest_ragged_f64 differs from the numpy specification")
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    piece = {"what": "one prg_nearest_ragged_f64 launch over both clouds of every scene, fp32 dataset against bf16 dataset; HIP "
                     "events around the launch, median after 3 warm-up launches; an evaluation = one candidate row against "
                     "one query row (8 float64 operations, a compare, 3 selects)",
             "device": torch.cuda.get_device_name(0), "scenes": a.scenes, "cloud_pairs": len(pairs), "rows": int(sizes.sum()),
             "largest_cloud": int(sizes.max()), "median_cloud": float(np.median(sizes)), "candidate_evaluations": evaluations,
             "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "repeats": a.repeats,
             "evaluations_per_s_median": evaluations / (med * 1e-3), "bit_identical_to_specification": True,
             "kernel_resources": KERNEL_RESOURCES}
    with open(a.out, "w") as f:
        json.dump(piece, f)
    print(json.dumps(piece), flush=True)


def run(a):
    work = tempfile.mkdtemp(prefix="dataset_equivalence_", dir=a.workdir)
    me = [sys.executable, os.path.abspath(__file__)]
    shape = ["--scenes", str(a.scenes), "--size", str(a.size), "--sampling-steps", str(a.sampling_steps), "--dim", str(a.dim),
             "--seed", str(a.seed), "--noise-seed", str(a.noise_seed)]
    d = lambda name: os.path.join(work, name)
    gen_limit = lambda dtype: int(2 * a.scenes / README_PAIRS_PER_S[dtype] * a.sampling_steps / 1000 * (a.size / 128) ** 2) + STARTUP_S
    steps = [(gen_limit("fp32"), me + ["generate", "--dtype", "fp32", "--batch", str(a.batch), "--out", d("fp32")] + shape)]
    steps += [(gen_limit(dt), me + ["generate", "--dtype", dt, "--batch", str(a.batch), "--out", d(dt)] + shape)
              for dt in ("bf16", "mxfp8", "f16x3")]
    steps += [(gen_limit("fp32"), me + ["generate", "--dtype", "fp32", "--batch", str(a.batch), "--lanes", "2", "--out",
                                       d("control")] + shape)]
    names = ("control", "f16x3", "bf16", "mxfp8")
    steps += [(120, me + ["compare", d("fp32"), d(n), "--scenes", str(a.scenes), "--out", d(n + ".json")]) for n in names]
    steps += [(120, me + ["kernel", d("fp32"), d("bf16"), "--scenes", str(a.scenes), "--repeats", str(a.repeats), "--out",
                          d("kernel.json")])]
    try:
        for limit, cmd in steps:
            print("+ timeout -k 10 {} {}".format(limit, " ".join(cmd[1:])), flush=True)
            t0 = time.perf_counter()
            rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=dict(os.environ, PYTHONPATH=ROOT)).returncode
            print("  -> exit {} after {:.0f} s".format(rc, time.perf_counter() - t0), flush=True)
            if rc != 0:
                raise SystemExit("step failed ({}): nothing more is started".format(rc))
        res = {"what": "the same {} synthetic scenes ({}x{}, dim {}, {} sampling steps of 1000, B = {}, synthetic seed {}, noise "
                       "seed {}, calibrated synthetic weights as bench.py's pipeline leg) generated in every arithmetic mode and "
                       "compared with the fp32 dataset cloud by cloud: distances in metres between nearest neighbours, both "
                       "directions; median / p95 / max are over the {} clouds".format(
                           a.scenes, a.size, a.size, a.dim, a.sampling_steps, a.batch, a.seed, a.noise_seed, 2 * a.scenes),
               "thresholds_m": {"0.0001": "north-star tolerance", "0.001": "1 mm", "0.0125": "half the save voxel",
                                "0.0375": "generate_gt's overlap radius"}, "comparisons": {}}
        for n in names:
            with open(d(n + ".json")) as f:
                res["comparisons"][n + "_vs_fp32"] = json.load(f)
        with open(d("kernel.json")) as f:
            res["nearest_launch"] = json.load(f)
        res["control_identical"] = res["comparisons"]["control_vs_fp32"]["summary"]["identical"]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="cmd", required=True)

    def shape(q):
        q.add_argument("--scenes", type=int, default=256)
        q.add_argument("--size", type=int, default=128)
        q.add_argument("--sampling-steps", type=int, default=1000)
        q.add_argument("--dim", type=int, default=64)
        q.add_argument("--seed", type=int, default=0, help="synthetic scene seed")
        q.add_argument("--noise-seed", type=int, default=0)
        q.add_argument("--batch", type=int, default=64)

    g = sub.add_parser("generate")
    shape(g)
    g.add_argument("--dtype", required=True, choices=sorted(README_PAIRS_PER_S))
    g.add_argument("--lanes", type=int, default=1)
    g.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    c.add_argument("--scenes", type=int, default=256)
    c.add_argument("--out", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("a")
    k.add_argument("b")
    k.add_argument("--scenes", type=int, default=256)
    k.add_argument("--repeats", type=int, default=11)
    k.add_argument("--out", required=True)
    r = sub.add_parser("run")
    shape(r)
    r.add_argument("--repeats", type=int, default=11)
    r.add_argument("--workdir", default=None, help="where the datasets are written (default: the system's temporary folder)")
    r.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_equivalence.json"))
    a = p.parse_args()
    {"generate": generate, "compare": compare, "kernel": kernel, "run": run}[a.cmd](a)


if __name__ == "__main__":
    main()
