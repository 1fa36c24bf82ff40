"""tools/predict.py --video on an npz holding frames_yuv with a pixel_format entry, in a child process: the track equals, array
for array (the overlay and the attention overlay included), that of the twin npz holding the converted frames_u8; an npz holding both kinds of pictures is refused."""
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
from csts_amd import inputs  # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
OPTS = ["NUM_GPUS", "1", "TEST.BATCH_SIZE", "3", "CSTS_AMD.COMPUTE", "fp32"]
PREDICT = os.path.join(ROOT, "tools", "predict.py")
N, H, W = 120, 64, 80


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _run(video, out, *more):
    cmd = [sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", "16", "--overlay", "--attention-overlay", "mean",
           "--out", out]
    return subprocess.run(cmd + list(more) + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)


def test_yuv_video_gives_the_track_of_its_rgb_twin(tmp_path):
    g = torch.Generator().manual_seed(21)
    yuv = torch.randint(0, 256, (N, H * 3 // 2, W), generator=g, dtype=torch.uint8).numpy()
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).numpy()
    paths = {k: (str(tmp_path / f"{k}.npz"), str(tmp_path / f"track_{k}.npz")) for k in ("yuv", "rgb", "flag")}
    np.savez(paths["yuv"][0], frames_yuv=yuv, pixel_format=np.array("i420"), yuv_matrix=np.array("bt709"), wav=wav)
    np.savez(paths["rgb"][0], frames_u8=inputs.yuv_to_rgb_host(yuv, "i420", "bt709"), wav=wav)
    np.savez(paths["flag"][0], frames_yuv=yuv, pixel_format=np.array("nv12"), wav=wav)      # the flags override the entries
    recs = {}
    for k, more in (("yuv", ()), ("rgb", ()), ("flag", ("--pixel-format", "i420", "--yuv-matrix", "bt709", "--yuv-full-range", "0"))):
        p = _run(*paths[k], *more)
        assert p.returncode == 0, p.stderr[-4000:]
        lines = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
        assert len(lines) == 1 and lines[0]["_type"] == "predict_video" and lines[0]["windows"] == 3
        recs[k] = lines[0]
    assert recs["yuv"]["pixel_format"] == recs["flag"]["pixel_format"] == "i420" and "pixel_format" not in recs["rgb"]
    assert recs["yuv"]["shapes"] == recs["rgb"]["shapes"] and recs["yuv"]["shapes"]["overlay"] == [N, H, W, 3]
    assert recs["yuv"]["shapes"]["attention_overlay"] == [N, H, W, 3]
    want = np.load(paths["rgb"][1])
    for k in ("yuv", "flag"):
        z = np.load(paths[k][1])
        assert sorted(z.files) == sorted(want.files)
        for name in want.files:
            assert z[name].dtype == want[name].dtype and np.array_equal(z[name], want[name], equal_nan=z[name].dtype.kind == "f"), name


def test_yuv_clip_gives_the_prediction_of_its_rgb_twin(tmp_path):
    B, T = 1, 8
    g = torch.Generator().manual_seed(22)
    yuv = torch.randint(0, 256, (B, T, H * 3 // 2, W), generator=g, dtype=torch.uint8).numpy()
    rest = dict(wav=(0.1 * torch.randn(B, 24000 * 5, generator=g)).numpy(),
                frames_idx=(np.arange(T, dtype=np.float32) + 0.5)[None].repeat(B, 0), frame_length=np.float64(T))
    np.savez(str(tmp_path / "yuv.npz"), frames_yuv=yuv, pixel_format=np.array("nv12"), **rest)
    np.savez(str(tmp_path / "rgb.npz"), frames_u8=inputs.yuv_to_rgb_host(yuv, "nv12"), **rest)
    for k in ("yuv", "rgb"):
        p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--clip", str(tmp_path / f"{k}.npz"), "--out",
                            str(tmp_path / f"gaze_{k}.npz")] + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-4000:]
        assert ('"pixel_format": "nv12"' in p.stdout) == (k == "yuv")
    got, want = np.load(str(tmp_path / "gaze_yuv.npz")), np.load(str(tmp_path / "gaze_rgb.npz"))
    assert sorted(got.files) == sorted(want.files) == ["heatmaps", "peak", "points", "rescaled"]
    for name in want.files:
        assert np.array_equal(got[name], want[name]), name


def test_an_npz_holding_both_kinds_of_pictures_is_refused(tmp_path):
    video = str(tmp_path / "both.npz")
    np.savez(video, frames_yuv=np.zeros((N, H * 3 // 2, W), np.uint8), pixel_format=np.array("nv12"),
             frames_u8=np.zeros((N, H, W, 3), np.uint8), wav=np.zeros(N * 800, np.float32))
    p = _run(video, str(tmp_path / "o.npz"))
    assert p.returncode != 0 and "holds both frames_u8 and frames_yuv" in p.stderr
    assert not os.path.exists(str(tmp_path / "o.npz"))
