"""validate_checkpoint.py end to end on the host (--device cpu: the specifications plus prg_cpu_unet_forward), in this process:
the table's shape, its JSON, the reference column, invariance under re-batching, and the mask metrics of caller-supplied pairs."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = ["--resume", "synthetic:3", "--device", "cpu", "--dim", "16", "--image_size", "32", "--synthetic_seed", "0", "-start", "2",
        "-stop", "5", "--timesteps", "0", "500", "999"]


def test_table_json_and_rebatching(tmp_path, capsys):
    import validate_checkpoint as vc
    assert vc.default_timesteps(1000) == sorted(set(vc.default_timesteps(1000))) and len(vc.default_timesteps(1000)) == 16
    assert vc.default_timesteps(1000)[0] == 0 and vc.default_timesteps(1000)[-1] == 999
    out = tmp_path / "a.json"
    res = vc.main(BASE + ["--batch_size", "2", "--out", str(out)])
    text = capsys.readouterr().out
    assert [r["t"] for r in res["rows"]] == [0, 500, 999] and json.load(open(out)) == res
    assert all(np.isfinite(r["fp32"]["loss"]) and r["fp32"]["minus_fp32"] == 0.0 for r in res["rows"])
    assert len([l for l in text.splitlines() if l.split() and l.split()[0] in ("0", "500", "999")]) == 3
    again = vc.main(BASE + ["--batch_size", "3", "--out", str(tmp_path / "b.json")])
    assert [r["fp32"]["loss"] for r in again["rows"]] == [r["fp32"]["loss"] for r in res["rows"]]      # keyed by scene, not by batch
    with pytest.raises(SystemExit):
        vc.main(BASE[:-3] + ["--timesteps", "1000"])
    with pytest.raises(SystemExit):
        vc.main(BASE + ["--dtypes", "fp32", "bf16"])


def test_mask_metrics_of_supplied_pairs(tmp_path):
    import validate_checkpoint as vc
    rng = np.random.default_rng(3)
    inp = rng.random((3, 32, 32), dtype=np.float32)
    lab = (inp + (rng.random((3, 32, 32), dtype=np.float32) - np.float32(0.5)) * np.float32(0.02)).astype(np.float32)
    np.savez(tmp_path / "pairs.npz", input=inp, label=lab)
    res = vc.main(BASE + ["--mask_milestone", "synthetic:4", "--mask_pairs", str(tmp_path / "pairs.npz"), "--batch_size", "2",
                          "--out", str(tmp_path / "m.json")])
    m = res["mask"]["fp32"]
    assert set(m) == {"MSE", "MAE", "SAE", "mIoU", "PAcc", "FP"} and all(np.isfinite(v) for v in m.values())
    assert 0 <= m["PAcc"] <= 1 and 0 <= m["mIoU"] <= 1 and m["MSE"] >= 0
