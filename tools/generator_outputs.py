#!/usr/bin/env python
"""Everything `Generator.generate`, `PairStream` and `Tester.generate` write or yield on a fixed case list, as sha256 digests,
for byte-for-byte A/B of two trees (a refactor of the Python orchestration against its parent).

  python tools/generator_outputs.py OUT.json [--tree DIR] [--device cpu]   # DIR: the checkout whose package runs (default: this one)
  python tools/generator_outputs.py --compare A.json B.json                # per case: identical or not; exit 1 on any difference

Every case runs at the configuration of tests/test_gpu_cloud_finish.py: S = 64, dim 16, 4 DDIM steps of 1000, batches of 2 over
4 scenes (so a resume marker is deferred across a batch boundary), synthetic seed = noise seed = 11, `mask_threshold=0.5`, fp32
synthetic weights.  Cases: `generate` for num_samples 1..3 x clouds fused / per_view x {voxel_backend host, device, gt_log}
(every file's path and digest); two lanes; a second run over a finished folder (the printed "Skip" lines, the unchanged tree);
`PairStream` fused, per view, per view with `Augment()` (every item field, `skipped`); `Tester.generate(4, 3)` on both backends
(the returned clouds, the files).  `--device cpu` runs the `voxel_backend="host"` generate cases alone, on `pointreggpt_amd.cpu`."""
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile

S, DIM, STEPS, BATCH, SCENES, SEED = 64, 16, 4, 2, 4, 11


def sha(data):
    return hashlib.sha256(data).hexdigest()


def tree(root):
    return {os.path.relpath(os.path.join(d, f), root): sha(open(os.path.join(d, f), "rb").read())
            for d, _dirs, files in os.walk(root) for f in files}


def value(v):
    """Digest of one item field: arrays and tensors by dtype, shape and bytes, the rest by repr."""
    import numpy as np
    import torch
    if isinstance(v, torch.Tensor):
        v = v.cpu().numpy()
    if isinstance(v, np.ndarray):
        return "{} {} {}".format(v.dtype, v.shape, sha(np.ascontiguousarray(v).tobytes()))
    return repr(v)


def run(out, device):
    import numpy as np
    from pointreggpt_amd.generator import Generator
    res = {}
    if device == "cpu":
        from pointreggpt_amd import cpu as M
        def nets():
            return (M.GaussianDiffusion(M.Unet(DIM).init_synthetic(3), image_size=S, timesteps=1000, sampling_timesteps=STEPS),
                    M.MaskUnet(DIM).init_synthetic(4, final_bias=8.0))
    else:
        from pointreggpt_amd.diffusion import GaussianDiffusion
        from pointreggpt_amd.unet import MaskUnet, Unet
        def nets():
            return (GaussianDiffusion(Unet(DIM, dtype="fp32").init_synthetic(3), image_size=S, timesteps=1000, sampling_timesteps=STEPS),
                    MaskUnet(DIM, dtype="fp32").init_synthetic(4, final_bias=8.0))
    diff, mask = nets()

    def generate(folder, ns, **kw):
        gen = Generator(diff, None, batch_size=BATCH, samples_folder=os.path.join(folder, "ds", "data"), synthetic_seed=SEED,
                        device="cpu" if device == "cpu" else "cuda")
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            gen.generate(0, SCENES, ns, depth_correction=mask, mask_threshold=0.5, noise_seed=SEED, **kw)
        return gen, printed.getvalue()

    with tempfile.TemporaryDirectory(prefix="prg_genout_") as tmp:
        backends = {"host": dict(voxel_backend="host")}
        if device != "cpu":
            backends.update(device=dict(voxel_backend="device"), gt_log=dict(gt_log=True))
        for ns in (1, 2, 3):
            for clouds in ("fused", "per_view"):
                for name, kw in backends.items():
                    case = "generate_ns{}_{}_{}".format(ns, clouds, name)
                    generate(os.path.join(tmp, case), ns, clouds=clouds, **kw)
                    res[case] = tree(os.path.join(tmp, case))
        if device != "cpu":
            generate(os.path.join(tmp, "lanes"), 2, clouds="per_view", gt_log=True, lanes=[nets()])
            res["generate_two_lanes"] = tree(os.path.join(tmp, "lanes"))
            again = os.path.join(tmp, "generate_ns2_per_view_gt_log")
            _gen, printed = generate(again, 2, clouds="per_view", gt_log=True)
            res["generate_resume"] = dict(tree(again), printed=printed)
            from pointreggpt_amd.stream import Augment, PairStream
            for case, kw in (("stream_fused_ns1", {}), ("stream_per_view_ns2", dict(num_samples=2, clouds="per_view")),
                             ("stream_per_view_ns2_augment", dict(num_samples=2, clouds="per_view", augment=Augment()))):
                gen = Generator(diff, None, batch_size=BATCH, samples_folder=os.path.join(tmp, case), synthetic_seed=SEED)
                stream = PairStream(gen, mask, start=0, stop=SCENES, noise_seed=SEED, mask_threshold=0.5, matching_radius=0.0375, **kw)
                items = list(stream)
                res[case] = {"item{}.{}".format(i, k): value(v) for i, it in enumerate(items) for k, v in sorted(it.items())}
                res[case]["skipped"] = repr(stream.skipped)
                res[case]["files"] = repr(tree(os.path.join(tmp, case)))
            from pointreggpt_amd.tester import Tester
            for backend in ("device", "host"):
                case = "tester_generate_" + backend
                np.random.seed(SEED)                                     # the intrinsics and turns come from numpy's legacy stream
                clouds = Tester(diff, batch_size=BATCH, samples_folder=os.path.join(tmp, case), seed=SEED).generate(4, 3, voxel_backend=backend)
                res[case] = dict(tree(os.path.join(tmp, case)),
                                 **{"cloud{}.{}".format(b, j): value(c) for b, batch in enumerate(clouds) for j, c in enumerate(batch)})
    json.dump(res, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps({"package": os.path.dirname(sys.modules["pointreggpt_amd"].__file__), "cases": len(res),
                      "digests": sum(len(v) for v in res.values()), "out": out}))


def compare(a, b):
    za, zb = json.load(open(a)), json.load(open(b))
    bad = sorted(set(za) ^ set(zb))
    for k in bad:
        print(f"{k:40s} only in one file")
    for k in sorted(set(za) & set(zb)):
        diff = sorted(n for n in set(za[k]) | set(zb[k]) if za[k].get(n) != zb[k].get(n))
        print(f"{k:40s} {len(za[k]):4d} digests  {'identical' if not diff else 'DIFFERENT: ' + ', '.join(diff[:4])}")
        if diff:
            bad.append(k)
    print(f"{len(za)} cases, {len(bad)} different")
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) == 3 and args[0] == "--compare":
        sys.exit(compare(args[1], args[2]))
    opts = {"--tree": os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "--device": "cuda"}
    while len(args) >= 3 and args[-2] in opts:
        opts[args[-2]] = args[-1]
        args = args[:-2]
    if len(args) != 1 or args[0].startswith("-") or opts["--device"] not in ("cuda", "cpu"):
        sys.exit(__doc__)
    sys.path.insert(0, os.path.abspath(opts["--tree"]))
    run(args[0], opts["--device"])
