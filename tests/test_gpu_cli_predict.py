"""Trained weights through the command line: tools/predict.py --checkpoint reproduces the saving model's gaze points in a fresh
process under another seed, and tools/run_net.py's test driver honours TEST.CHECKPOINT_FILE_PATH (the reference's
load_test_checkpoint, tools/test_avgaze_net.py:120): its single test record is the metric of the saved weights."""
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
sys.path.insert(0, ROOT)
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
OPTS = ["NUM_GPUS", "1", "TEST.BATCH_SIZE", "2", "MODEL.LOSS_FUNC", "kldiv+egonce", "TRAIN.MIXED_PRECISION", "True"]
DEV = torch.device("cuda:0")


class _NoOptimizer:
    def state_dict(self):
        return {}


def _child(cmd, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]            # nothing is started after a failing child
    return [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]


def _six(v):
    return float(f"{v:.6g}")                               # what cli._log prints


def test_predict_and_test_driver_use_the_checkpoint(tmp_path):
    from csts_amd import checkpoint as ck, losses, metrics, train as T
    from csts_amd.build import build_model
    from csts_amd.config import load_yaml
    from csts_amd.infer import eval_forward
    cfg = load_yaml(YAML, OPTS + ["RNG_SEED", "11"])
    torch.manual_seed(11)
    model = build_model(cfg)
    model.eval()
    batch = T.synthetic_batch(2, cfg.DATA.NUM_FRAMES, cfg.DATA.TEST_CROP_SIZE, 2000, DEV)
    with torch.no_grad():
        mine = eval_forward(model, batch["video"], batch["audio"])
        preds = losses.frame_softmax(model([batch["video"]], batch["audio"]), temperature=2)
        want = metrics.adaptive_f1(preds, batch["labels_hm"], batch["labels"], dataset=cfg.TEST.DATASET, rescale=True)
        preds_sum = float(preds.sum())
    points = mine["points"].cpu().numpy()
    path = ck.save_checkpoint(str(tmp_path), model, _NoOptimizer(), 0, cfg)
    del model, mine, preds
    torch.cuda.empty_cache()
    try:
        out = str(tmp_path / "gaze.npz")
        recs = _child([sys.executable, os.path.join(ROOT, "tools", "predict.py"), "--cfg", YAML, "--checkpoint", path, "--seed", "2000",
                       "--batch", "2", "--out", out] + OPTS + ["RNG_SEED", "12"], timeout=900)
        assert len(recs) == 1 and recs[0]["_type"] == "predict" and recs[0]["checkpoint"] == path
        T_ = cfg.DATA.NUM_FRAMES
        assert recs[0]["shapes"] == {"points": [2, T_, 2], "peak": [2, T_], "rescaled": [2, T_, 64, 64], "heatmaps": [2, T_, 64, 64]}
        z = np.load(out)
        assert sorted(z.files) == ["heatmaps", "peak", "points", "rescaled"]
        assert z["points"].dtype == np.float32 and np.array_equal(z["points"], points)
        # without --checkpoint and another seed the points are other weights' points
        out2 = str(tmp_path / "gaze_random.npz")
        recs = _child([sys.executable, os.path.join(ROOT, "tools", "predict.py"), "--cfg", YAML, "--seed", "2000", "--batch", "2",
                       "--out", out2] + OPTS + ["RNG_SEED", "12"], timeout=900)
        assert recs[0]["checkpoint"] is None and not np.array_equal(np.load(out2)["points"], points)
        # the test driver: one test record, the metric of the SAVED weights to the printed six digits
        recs = _child([sys.executable, os.path.join(ROOT, "tools", "run_net.py"), "--cfg", YAML] + OPTS +
                      ["RNG_SEED", "12", "TRAIN.ENABLE", "False", "TEST.ENABLE", "True", "TEST.CHECKPOINT_FILE_PATH", path,
                       "OUTPUT_DIR", str(tmp_path / "job")], timeout=900)
        tests = [r for r in recs if r["_type"] == "test"]
        assert len(tests) == 1 and [r["_type"] for r in recs] == ["test"]
        r = tests[0]
        assert set(r) == {"_type", "preds_shape", "preds_sum", "f1", "recall", "precision", "threshold"}
        print("test record", r, "in-process", want)
        assert r["f1"] == _six(want[0]) and r["recall"] == _six(want[1]) and r["precision"] == _six(want[2])
        assert r["threshold"] == _six(float(want[3])) and abs(r["preds_sum"] - preds_sum) < 1e-3
    finally:
        os.remove(path)                                    # 0.75 GB
