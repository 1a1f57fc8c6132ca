"""Compare two generated datasets cloud by cloud: is this the same dataset, only faster?

Two trees written by `generate_dataset.py` (or `Generator.generate`) from the same scenes — same `--synthetic` seed and
`--noise_seed`, so that poses and noise do not depend on dtype, batch or lane — are compared by what a user of the clouds
sees: for every `data/scene-XXXXXX/sample-XXXXXX.cloud.ply` present in both, the nearest-neighbour distances between the
two clouds in both directions (`postprocess.cloud_distance_metrics`: Chamfer, Hausdorff, percentiles, shares within the
tolerances that matter here), and for every `gt.log` line present in both the change of the two overlap ratios.  Nothing
here is indexed by pixel, so it is well defined when the valid masks of the two runs differ.

The distances of up to `scenes_per_launch` scenes come from ONE prg_nearest_ragged_f64 launch (exact float64 all-pairs
search).  `backend="numpy-spec"` runs the numpy specification `postprocess.nearest` instead: like
`generate_gt(overlap="numpy-spec")` a test hook for machines without a GPU, never chosen implicitly.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import postprocess as PP

METRICS = ("chamfer", "hausdorff", "p50", "p95", "p99")


def _cloud_path(root: Path, scene: int, sample: int) -> Path:
    return root / "data" / "scene-{:0>6d}".format(scene) / "sample-{:0>6d}.cloud.ply".format(sample)


def read_gt(root, start: int, stop: int) -> Dict[Tuple[int, int, int], Tuple[float, float]]:
    """(scene, s, t) -> (overlap_src, overlap_tgt) of the scenes [start, stop): from `metadata/gt.log` if the tree has one,
    otherwise from the scenes' own `gt.log` files."""
    root = Path(root)
    gathered = root / "metadata" / "gt.log"
    if gathered.is_file():
        files = [gathered]
    else:
        files = [root / "data" / "scene-{:0>6d}".format(i) / "gt.log" for i in range(start, stop)]
    out = {}
    for f in files:
        if not f.is_file():
            continue
        for line in f.read_text().splitlines():
            tok = line.split()
            if len(tok) < 5:
                continue
            scene = int(tok[0].rsplit("-", 1)[1])
            if start <= scene < stop:
                out[(scene, int(tok[1]), int(tok[2]))] = (float(tok[3]), float(tok[4]))
    return out


def _spread(values) -> dict:
    """Median, p95 and max of a list of per-scene values (NaN when there are none)."""
    v = np.asarray(list(values), dtype=np.float64)
    if len(v) == 0:
        return {"median": float("nan"), "p95": float("nan"), "max": float("nan")}
    return {"median": float(np.median(v)), "p95": float(np.percentile(v, 95)), "max": float(v.max())}


def _nearest(pairs, backend: str):
    if backend == "hip":
        return PP.nearest_hip(pairs)
    out = []
    for a, b in pairs:
        d2_ab, i_ab = PP.nearest(a, b)
        d2_ba, i_ba = PP.nearest(b, a)
        out.append((d2_ab, i_ab, d2_ba, i_ba))
    return out


def compare_datasets(root_a, root_b, start: int, stop: int, samples: Sequence[int] = (0, 1), scenes_per_launch: int = 256,
                     backend: str = "hip", thresholds: Sequence[float] = PP.DISTANCE_THRESHOLDS) -> dict:
    """Compare the scenes [start, stop) of the dataset trees `root_a` and `root_b` (each holds `data/` and possibly
    `metadata/`).  Returns the report:

      clouds   one entry per (scene, sample): {"scene", "sample", "missing_a", "missing_b"} and, where both files exist,
               the metrics of `postprocess.cloud_distance_metrics` (with `within` keyed by the threshold's repr)
      gt       {"common", "only_a", "only_b", "lines": [{"scene", "s", "t", "d_overlap_src", "d_overlap_tgt"}, ...]}
      summary  counts (compared, missing_a, missing_b, empty, gt_common, gt_only_a, gt_only_b), median / p95 / max over the
               compared non-empty clouds of every metric, the same for |d_overlap_src| and |d_overlap_tgt|, `identical`:
               at least one cloud pair was compared and every one has equal row counts and a Hausdorff distance of 0, and
               `by_sample`: the same spreads (plus the smallest `within` share) over the clouds of one sample index each.

    A file missing on either side is recorded and counted, and left out of the aggregates."""
    if backend not in ("hip", "numpy-spec"):
        raise ValueError("backend must be 'hip' or 'numpy-spec'")
    if scenes_per_launch < 1:
        raise ValueError("scenes_per_launch < 1")
    root_a, root_b = Path(root_a), Path(root_b)
    thresholds = tuple(float(t) for t in thresholds)
    clouds, pending = [], []                        # pending: (entry, cloud of a, cloud of b) of the scenes of one launch

    def flush():
        res = _nearest([(a, b) for _e, a, b in pending], backend) if pending else []
        for (entry, _a, _b), (d2_ab, _i_ab, d2_ba, _i_ba) in zip(pending, res):
            m = PP.cloud_distance_metrics(d2_ab, d2_ba, thresholds)
            m["within"] = {repr(t): v for t, v in m["within"].items()}
            entry.update(m)
        pending.clear()

    for n, scene in enumerate(range(start, stop)):
        if n and n % scenes_per_launch == 0:
            flush()
        for k in samples:
            pa, pb = _cloud_path(root_a, scene, k), _cloud_path(root_b, scene, k)
            entry = {"scene": scene, "sample": int(k), "missing_a": not pa.is_file(), "missing_b": not pb.is_file()}
            clouds.append(entry)
            if not (entry["missing_a"] or entry["missing_b"]):
                pending.append((entry, PP.read_ply(str(pa)), PP.read_ply(str(pb))))
    flush()

    gt_a, gt_b = read_gt(root_a, start, stop), read_gt(root_b, start, stop)
    lines = [{"scene": key[0], "s": key[1], "t": key[2], "d_overlap_src": abs(gt_a[key][0] - gt_b[key][0]),
              "d_overlap_tgt": abs(gt_a[key][1] - gt_b[key][1])} for key in sorted(gt_a.keys() & gt_b.keys())]
    gt = {"common": len(lines), "only_a": len(gt_a.keys() - gt_b.keys()), "only_b": len(gt_b.keys() - gt_a.keys()),
          "lines": lines}

    compared = [e for e in clouds if "n_a" in e]
    measured = [e for e in compared if not e["empty"]]
    summary = {"compared": len(compared), "missing_a": sum(e["missing_a"] for e in clouds),
               "missing_b": sum(e["missing_b"] for e in clouds), "empty": len(compared) - len(measured),
               "gt_common": gt["common"], "gt_only_a": gt["only_a"], "gt_only_b": gt["only_b"]}
    for name in METRICS:
        summary[name] = _spread(e[name] for e in measured)
    for t in thresholds:
        summary["within[{!r}]".format(t)] = _spread(e["within"][repr(t)] for e in measured)
    summary["d_overlap_src"] = _spread(ln["d_overlap_src"] for ln in lines)
    summary["d_overlap_tgt"] = _spread(ln["d_overlap_tgt"] for ln in lines)
    same = lambda e: e["n_a"] == e["n_b"] and (e["n_a"] == 0 or e["hausdorff"] == 0)
    summary["identical"] = bool(compared) and all(same(e) for e in compared)
    # the same per sample index: sample 0 is the scene's memory cloud (it never went through the networks with one view per
    # scene), so an aggregate over all clouds mixes clouds that cannot differ with those that can
    summary["by_sample"] = {}
    for k in samples:
        mine = [e for e in measured if e["sample"] == int(k)]
        part = {"compared": sum(e["sample"] == int(k) for e in compared),
                "identical_clouds": sum(same(e) for e in compared if e["sample"] == int(k))}
        for name in METRICS:
            part[name] = _spread(e[name] for e in mine)
        for t in thresholds:
            w = [e["within"][repr(t)] for e in mine]
            part["within[{!r}]".format(t)] = dict(_spread(w), min=float(min(w)) if w else float("nan"))
        summary["by_sample"][str(int(k))] = part
    return {"root_a": str(root_a), "root_b": str(root_b), "start": int(start), "stop": int(stop),
            "samples": [int(k) for k in samples], "backend": backend, "thresholds": list(thresholds),
            "summary": summary, "gt": gt, "clouds": clouds}


def main(argv: Optional[Sequence[str]] = None) -> dict:
    """compare_datasets.py A B -start I -stop J [--out report.json]: prints the summary as one JSON line, writes the report."""
    import argparse
    p = argparse.ArgumentParser(description="Compare two generated datasets: nearest-neighbour cloud distances and gt.log")
    p.add_argument("root_a", help="dataset tree A (the directory that holds data/ and metadata/)")
    p.add_argument("root_b", help="dataset tree B")
    p.add_argument("--start_scene_index", "-start", default=0, type=int)
    p.add_argument("--stop_scene_index", "-stop", default=1, type=int)
    p.add_argument("--samples", default=[0, 1], type=int, nargs="+", help="sample indices compared per scene")
    p.add_argument("--scenes_per_launch", default=256, type=int)
    p.add_argument("--backend", default="hip", choices=["hip", "numpy-spec"],
                   help="numpy-spec = the numpy specification instead of the HIP kernel (test hook, explicit only)")
    p.add_argument("--out", default="dataset_comparison.json", type=str, help="where the full report is written")
    args = p.parse_args(argv)
    report = compare_datasets(args.root_a, args.root_b, args.start_scene_index, args.stop_scene_index, samples=args.samples,
                              scenes_per_launch=args.scenes_per_launch, backend=args.backend)
    print(json.dumps(report["summary"]))
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    return report
