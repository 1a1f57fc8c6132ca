"""generate_dataset.py --objective / --beta_schedule: the two flags reach GaussianDiffusion, on the CPU twins here and on the device
under `-m gpu`; without them the command line means what it meant."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--resume", "synthetic:3", "--synthetic", "1", "--dim", "16", "--image_size", "32", "--timesteps", "1000",
          "--sampling_timesteps", "5", "--batch_size", "2", "-start", "0", "-stop", "2", "--noise_seed", "5", "--dtype", "fp32"]


def generate(cwd, name, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_dataset.py"), *COMMON, "--dataset_name", name, *flags], cwd=cwd,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for scene in ("scene-000000", "scene-000001"):
        with open(os.path.join(cwd, name, "data", scene, "sample-000001.cloud.ply"), "rb") as f:
            out[scene] = f.read()
        assert len(out[scene]) > 1000
    return out


def check(tmp_path, device):
    v = generate(str(tmp_path), "v_linear", "--device", device, "--objective", "pred_v", "--beta_schedule", "linear")
    default = generate(str(tmp_path), "default", "--device", device)
    spelled = generate(str(tmp_path), "spelled", "--device", device, "--objective", "pred_x0", "--beta_schedule", "sigmoid")
    assert default == spelled and v != default


def test_flags_reach_the_cpu_twin(tmp_path):
    check(tmp_path, "cpu")


def test_unknown_names_are_refused_by_the_parser(tmp_path):
    for flags in (["--objective", "pred_eps"], ["--beta_schedule", "quadratic"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_dataset.py"), *COMMON, "--device", "cpu", *flags], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 2 and "invalid choice" in r.stderr


@pytest.mark.gpu
def test_flags_reach_the_device(tmp_path):
    check(tmp_path, "cuda")
