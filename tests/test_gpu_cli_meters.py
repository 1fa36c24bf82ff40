"""CSTS_AMD.GAZE_METERS through the advertised entry point (tools/run_net.py in a fresh child process): with the switch the
train_iter / train_epoch / val_epoch records carry the meter's values and exactly one test_final record follows the test
record; without it the records carry the keys they carried before the meters existed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS_BEFORE = {
    "train_start": {"_type", "start_epoch", "resumed", "optimizer_steps"},
    "train_iter": {"_type", "epoch", "iter", "lr", "lr_device", "loss_scale", "loss", "kldiv_loss", "nce_loss"},
    "train_epoch": {"_type", "epoch", "clips_per_s"},
    "val_epoch": {"_type", "epoch", "f1", "recall", "precision", "iters"},
    "test": {"_type", "preds_shape", "preds_sum", "f1", "recall", "precision", "threshold"},
}


def _run_net(out_dir, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_net.py"), "--cfg", os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
           "NUM_GPUS", "1", "TRAIN.BATCH_SIZE", "2", "TEST.BATCH_SIZE", "2", "MODEL.LOSS_FUNC", "kldiv+egonce", "MODEL.LOSS_ALPHA", "0.05",
           "TRAIN.MIXED_PRECISION", "True", "CSTS_AMD.STEPS_PER_EPOCH", "4", "TRAIN.EVAL_PERIOD", "1", "CSTS_AMD.EPOCHS_THIS_RUN", "1",
           "LOG_PERIOD", "2", "OUTPUT_DIR", str(out_dir)] + list(extra)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    return [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]


def _unit(r, keys):
    for k in keys:
        assert np.isfinite(r[k]) and 0.0 <= r[k] <= 1.0, (k, r)


def test_run_net_with_gaze_meters(tmp_path):
    recs = _run_net(tmp_path, ["CSTS_AMD.GAZE_METERS", "True", "CSTS_AMD.TEST_STEPS", "3"])
    kinds = [r["_type"] for r in recs]
    iters = [r for r in recs if r["_type"] == "train_iter"]
    assert [r["iter"] for r in iters] == [2, 4]
    for r in iters:
        assert set(r) == KEYS_BEFORE["train_iter"] | {"f1", "recall", "precision", "threshold"}
        _unit(r, ("f1", "recall", "precision"))
        assert 0.01 - 1e-9 <= r["threshold"] <= 0.07 + 1e-9
    ep = [r for r in recs if r["_type"] == "train_epoch"]
    assert len(ep) == 1 and set(ep[0]) == KEYS_BEFORE["train_epoch"] | {"f1", "recall", "precision"}
    _unit(ep[0], ("f1", "recall", "precision"))
    val = [r for r in recs if r["_type"] == "val_epoch"]
    assert len(val) == 1 and set(val[0]) == KEYS_BEFORE["val_epoch"]
    # synthetic clips carry gaze type 0 only, so no frame has the type ValGazeMeter weighs with (labels[:, 2] == 1): zero
    # samples, where the reference divides by zero and this meter reports NaN
    assert all(np.isnan(val[0][k]) for k in ("f1", "recall", "precision"))
    assert kinds.count("test") == 1 and kinds.count("test_final") == 1 and kinds.index("test_final") == kinds.index("test") + 1
    final = recs[kinds.index("test_final")]
    assert set(final) == {"_type", "recall", "precision", "f1", "threshold", "iters"} and final["iters"] == 3
    _unit(final, ("f1", "recall", "precision"))
    assert set(recs[kinds.index("test")]) == KEYS_BEFORE["test"]


def test_run_net_without_the_key_prints_the_same_record_keys(tmp_path):
    recs = _run_net(tmp_path)
    kinds = [r["_type"] for r in recs]
    assert "test_final" not in kinds and set(kinds) == set(KEYS_BEFORE)
    for r in recs:
        assert set(r) == KEYS_BEFORE[r["_type"]], r
    _unit([r for r in recs if r["_type"] == "val_epoch"][0], ("f1", "recall", "precision"))
