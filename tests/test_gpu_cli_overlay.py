"""tools/predict.py --video --overlay in a child process: the npz gains the rendered recording and the source-frame points;
without the flag its entries are the ones tests/test_gpu_cli_predict_video.py lists."""
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
N, H, W = 200, 64, 80
TRACK = ["count", "heatmaps", "peak", "points", "rescaled"]


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _run(tmp_path, name, extra):
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).numpy()
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).numpy()
    video, out = str(tmp_path / "video.npz"), str(tmp_path / name)
    np.savez(video, frames_u8=frames, wav=wav, fps=np.float64(30.0))
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", "16", "--out", out] + extra + OPTS,
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(recs) == 1 and recs[0]["_type"] == "predict_video"
    return frames, np.load(out), recs[0]


def test_overlay_flag_adds_the_rendered_recording(tmp_path):
    frames, z, rec = _run(tmp_path, "track.npz", ["--overlay"])
    assert sorted(z.files) == sorted(TRACK + ["overlay", "points_source"])
    assert z["overlay"].dtype == np.uint8 and z["overlay"].shape == (N, H, W, 3) and rec["shapes"]["overlay"] == [N, H, W, 3]
    assert z["points_source"].shape == (N, 2) and z["points_source"].dtype == np.float64
    covered = z["count"] > 0
    assert 0 < covered.sum() < N
    assert np.array_equal(z["overlay"][~covered], frames[~covered])
    assert (z["overlay"][covered] != frames[covered]).reshape(int(covered.sum()), -1).any(axis=1).all()
    assert np.isnan(z["points_source"][~covered]).all() and np.isfinite(z["points_source"][covered]).all()


def test_without_the_flag_the_file_list_is_unchanged(tmp_path):
    _, z, rec = _run(tmp_path, "plain.npz", [])
    assert sorted(z.files) == TRACK and sorted(rec["shapes"]) == TRACK


def test_overlay_needs_a_video(tmp_path):
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--overlay", "--out", str(tmp_path / "o.npz")] + OPTS, cwd=ROOT,
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and p.stdout.strip() == "" and "need --video" in p.stderr
