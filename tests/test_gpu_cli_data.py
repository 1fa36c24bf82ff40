"""run_net.py on recorded clips (CSTS_AMD.SYNTHETIC_DATA False + CSTS_AMD.DATA_ROOT) in a child process: one epoch over a toy
train split of 4 clips of 64 x 80 frames at batch 2 logs two train_iter records with finite loss, a val_epoch over the val
split and, with TEST.ENABLE, a test_final whose iters is the number of test batches; without DATA_ROOT it is a config error."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_toy_dataset import write_dataset  # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
RUN = os.path.join(ROOT, "tools", "run_net.py")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _run(tmp_path, *opts):
    cmd = [sys.executable, RUN, "--cfg", YAML, "NUM_GPUS", "1", "OUTPUT_DIR", str(tmp_path / "out"), "TRAIN.BATCH_SIZE", "2",
           "TEST.BATCH_SIZE", "2", "SOLVER.MAX_EPOCH", "1", "LOG_PERIOD", "1", "CSTS_AMD.SYNTHETIC_DATA", "False"] + list(opts)
    return subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)


def test_train_val_test_on_a_toy_data_set(tmp_path):
    root = str(tmp_path / "toy")
    write_dataset(root, clips_per_video=(2, 2), sizes=((64, 80),), test_clips=3, seed=2)
    p = _run(tmp_path, "CSTS_AMD.DATA_ROOT", root, "TEST.ENABLE", "True")
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    by = {}
    for r in recs:
        by.setdefault(r["_type"], []).append(r)
    data = {r["split"]: r for r in by["data"]}
    assert data["train"]["clips"] == 4 and data["train"]["steps_per_epoch"] == 2 and data["val"]["clips"] == 3
    assert len(by["train_iter"]) == 2 and all(math.isfinite(r["loss"]) for r in by["train_iter"])
    assert [r["iter"] for r in by["train_iter"]] == [1, 2]
    assert len(by["train_epoch"]) == 1 and by["train_epoch"][0]["replaced_clips"] == 0
    assert len(by["val_epoch"]) == 1 and by["val_epoch"][0]["iters"] == 2 and 0.0 <= by["val_epoch"][0]["f1"] <= 1.0
    assert len(by["test_final"]) == 1 and by["test_final"][0]["iters"] == 2 and by["test_final"][0]["clips"] == 3
    assert 0.0 <= by["test_final"][0]["f1"] <= 1.0


def test_recorded_clips_need_a_data_root(tmp_path):
    p = _run(tmp_path)
    assert p.returncode != 0 and "config error" in p.stderr and "CSTS_AMD.DATA_ROOT" in p.stderr
    assert "train_iter" not in p.stdout
