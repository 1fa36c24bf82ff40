"""tools/predict.py --video in a child process: a small recording in, the per-frame track out, one predict_video json_stats
line; --video together with --clip is refused."""
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
OPTS = ["NUM_GPUS", "1", "TEST.BATCH_SIZE", "3", "CSTS_AMD.COMPUTE", "fp32"]
PREDICT = os.path.join(ROOT, "tools", "predict.py")
N = 200


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def test_video_in_track_out(tmp_path):
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N, 64, 80, 3), generator=g, dtype=torch.uint8).numpy()
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).numpy()
    video, out = str(tmp_path / "video.npz"), str(tmp_path / "track.npz")
    np.savez(video, frames_u8=frames, wav=wav, fps=np.float64(30.0))
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", "16", "--out", out] + OPTS,
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(recs) == 1 and recs[0]["_type"] == "predict_video" and recs[0]["source"] == video
    assert recs[0]["windows"] == 8 and recs[0]["frames"] == N and 0 < recs[0]["covered_frames"] < N
    shapes = {"points": [N, 2], "peak": [N], "count": [N], "rescaled": [N, 64, 64], "heatmaps": [N, 64, 64]}
    assert recs[0]["shapes"] == shapes
    z = np.load(out)
    assert sorted(z.files) == sorted(shapes) and all(list(z[k].shape) == v for k, v in shapes.items())
    assert z["count"].dtype == np.int32 and int((z["count"] > 0).sum()) == recs[0]["covered_frames"]
    assert np.isnan(z["points"][z["count"] == 0]).all() and np.isfinite(z["points"][z["count"] > 0]).all()


def test_video_and_clip_exclude_each_other(tmp_path):
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--video", str(tmp_path / "v.npz"), "--clip", str(tmp_path / "c.npz"),
                        "--out", str(tmp_path / "o.npz")] + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and p.stdout.strip() == "" and "exclude each other" in p.stderr
