"""tools/predict.py --video --attention-track / --attention-overlay in child processes: the .npz gains exactly the attention
track's arrays and the predict_video record its two fields; without the flags the keys are what they were."""
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
BASE = {"points", "peak", "count", "rescaled", "heatmaps"}
TRACK = {"attention_maps", "attention_range", "attention_mixed", "attention_count", "temporal_attention_windows"}


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


@pytest.fixture(scope="module")
def video(tmp_path_factory):
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).numpy()
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).numpy()
    path = str(tmp_path_factory.mktemp("recording") / "video.npz")
    np.savez(path, frames_u8=frames, wav=wav, fps=np.float64(30.0))
    return path, frames


def _predict(video, out, *flags):
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", "16", "--out", out, *flags] + OPTS,
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(recs) == 1 and recs[0]["_type"] == "predict_video"
    return recs[0], np.load(out)


def test_the_track_adds_exactly_its_arrays_and_two_record_fields(video, tmp_path):
    path, _ = video
    plain, zp = _predict(path, str(tmp_path / "plain.npz"), "--no-graph")
    rec, z = _predict(path, str(tmp_path / "track.npz"), "--attention-track")
    assert set(zp.files) == BASE and set(z.files) == BASE | TRACK
    assert set(rec) - set(plain) == {"attention_track", "attention_frames"} and set(plain) - set(rec) == set()
    assert "attention_track" not in plain and rec["attention_track"] is True
    heads = z["attention_maps"].shape[1] - 1
    h, w = z["attention_maps"].shape[2:]
    assert heads >= 1 and z["attention_maps"].shape == z["attention_mixed"].shape == (N, heads + 1, h, w)
    assert z["attention_range"].shape == (N, heads + 1, 2) and z["attention_count"].shape == (N,)
    assert z["attention_count"].dtype == np.int32
    tw = z["temporal_attention_windows"]
    assert tw.ndim == 3 and tw.shape[0] == rec["windows"] == 8 and tw.shape[1] == tw.shape[2]
    hit = z["attention_count"] > 0
    assert rec["attention_frames"] == int(hit.sum()) and 0 < rec["attention_frames"] < N
    assert np.isnan(z["attention_range"][~hit]).all() and np.isfinite(z["attention_range"][hit]).all()
    assert rec["shapes"] == {k: list(z[k].shape) for k in z.files}
    for k in BASE:                                                # graph with the track against eager without it
        assert np.array_equal(np.nan_to_num(z[k], nan=-1.0), np.nan_to_num(zp[k], nan=-1.0)), k


def test_the_overlay_implies_the_track_and_adds_the_picture(video, tmp_path):
    path, frames = video
    rec, z = _predict(path, str(tmp_path / "drawn.npz"), "--attention-overlay", "mean", "--fill", "hold", "--no-graph")
    assert set(z.files) == BASE | TRACK | {"neighbours", "filled", "attention_neighbours", "attention_filled", "attention_overlay"}
    assert rec["attention_track"] is True
    drawn = (z["attention_count"] > 0) | z["attention_filled"]
    assert rec["attention_frames"] == int(drawn.sum()) and int(z["attention_filled"].sum()) > 0
    picture = z["attention_overlay"]
    assert picture.shape == (N, H, W, 3) and picture.dtype == np.uint8
    assert np.array_equal(picture[~drawn], frames[~drawn]) and int((~drawn).sum()) > 0
    assert all((picture[n] != frames[n]).any() for n in np.flatnonzero(drawn))
