#!/usr/bin/env python
"""compare_datasets.py — how far apart are two generated datasets?

    python compare_datasets.py ./dataset_fp32 ./dataset_bf16 -start 0 -stop 256 [--out report.json]

A and B are dataset trees as `generate_dataset.py` writes them (the directories that hold data/ and metadata/), generated
from the same scenes (`--synthetic SEED --noise_seed N` make a scene's poses and noise independent of dtype, batch and lane).
For every sample-XXXXXX.cloud.ply present in both: nearest-neighbour distances in both directions (one HIP launch per
`--scenes_per_launch` scenes) -> Chamfer, Hausdorff, p50 / p95 / p99 and the shares within 0.1 mm, 1 mm, half the save voxel
and generate_gt's overlap radius; for every gt.log line present in both: the change of the overlap ratios.  Prints the
summary (median / p95 / max over scenes, the counts of missing files and one-sided gt.log lines, `identical`) as one JSON
line and writes the full per-cloud report to --out.
"""
from pointreggpt_amd.compare import main

if __name__ == "__main__":
    main()
