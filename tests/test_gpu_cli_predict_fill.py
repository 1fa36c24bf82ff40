"""tools/predict.py --video --fill in a child process: the track comes back filled, with neighbours and filled in the .npz and
fill, max_gap and filled_frames in the predict_video record; --fill without --video and --max-gap without --fill are refused
before anything is printed."""
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


def test_video_in_filled_track_out(tmp_path):
    from csts_amd import fill_plan
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N, 64, 80, 3), generator=g, dtype=torch.uint8).numpy()
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).numpy()
    video, out = str(tmp_path / "video.npz"), str(tmp_path / "track.npz")
    np.savez(video, frames_u8=frames, wav=wav, fps=np.float64(30.0))
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", "16", "--fill", "linear", "--out", out]
                       + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(recs) == 1 and recs[0]["_type"] == "predict_video" and recs[0]["source"] == video
    assert recs[0]["windows"] == 8 and recs[0]["frames"] == N and 0 < recs[0]["covered_frames"] < N
    assert recs[0]["fill"] == "linear" and recs[0]["max_gap"] == 9 and recs[0]["filled_frames"] > 0
    shapes = {"points": [N, 2], "peak": [N], "count": [N], "rescaled": [N, 64, 64], "heatmaps": [N, 64, 64],
              "neighbours": [N, 2], "filled": [N]}
    assert recs[0]["shapes"] == shapes
    z = np.load(out)
    assert sorted(z.files) == sorted(shapes) and all(list(z[k].shape) == v for k, v in shapes.items())
    count, filled, nb = z["count"], z["filled"], z["neighbours"]
    assert count.dtype == np.int32 and nb.dtype == np.int32 and filled.dtype == np.bool_
    assert int((count > 0).sum()) == recs[0]["covered_frames"] and int(filled.sum()) == recs[0]["filled_frames"]
    assert np.array_equal(nb.astype(np.int64), fill_plan(count, 9))
    assert np.array_equal(filled, (count == 0) & (nb[:, 0] >= 0))
    assert np.isfinite(z["points"][filled]).all() and np.isfinite(z["points"][count > 0]).all()
    assert np.isnan(z["points"][(count == 0) & ~filled]).all()
    assert (z["peak"][filled] > 0).all() and np.abs(z["heatmaps"][filled].astype(np.float64).sum(axis=(1, 2)) - 1.0).max() <= 1e-5


def test_fill_needs_a_video_and_max_gap_needs_fill(tmp_path):
    out = str(tmp_path / "o.npz")
    for extra, word in ((["--fill", "linear"], "needs --video"), (["--video", str(tmp_path / "v.npz"), "--max-gap", "5"], "needs --fill")):
        p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--out", out] + extra + OPTS, cwd=ROOT, env=_env(),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and p.stdout.strip() == "" and word in p.stderr, (extra, p.stderr[-2000:])
        assert not os.path.exists(out)
