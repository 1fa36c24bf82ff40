"""tools/predict.py --video on an npz holding padded 4:2:0 surfaces (frames_yuv with a yuv_window entry), in a child process: the
track equals, array for array, that of the npz holding the repacked pictures; the output npz and the json_stats line carry
yuv_window; --yuv-window overrides the entry; the flag on an npz of packed RGB is refused."""
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
N, HS, WS = 120, 72, 96
WINDOW = (4, 6, 64, 80)


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _run(video, out, *more):
    cmd = [sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", "16", "--overlay", "--out", out]
    return subprocess.run(cmd + list(more) + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)


def test_surfaces_give_the_track_of_the_repacked_recording(tmp_path):
    g = torch.Generator().manual_seed(24)
    surf = torch.randint(0, 256, (N, HS * 3 // 2, WS), generator=g, dtype=torch.uint8).numpy()
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).numpy()
    fmt = dict(pixel_format=np.array("i420"), yuv_matrix=np.array("bt709"), wav=wav)
    paths = {k: (str(tmp_path / f"{k}.npz"), str(tmp_path / f"track_{k}.npz")) for k in ("entry", "tight", "flag")}
    np.savez(paths["entry"][0], frames_yuv=surf, yuv_window=np.asarray(WINDOW), **fmt)
    np.savez(paths["tight"][0], frames_yuv=inputs.yuv_window(surf, "i420", WINDOW), **fmt)
    np.savez(paths["flag"][0], frames_yuv=surf, yuv_window=np.asarray((0, 0, HS, WS)), **fmt)      # the flag overrides the entry
    recs = {}
    for k, more in (("entry", ()), ("tight", ()), ("flag", ("--yuv-window",) + tuple(str(v) for v in WINDOW))):
        p = _run(*paths[k], *more)
        assert p.returncode == 0, p.stderr[-4000:]
        lines = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
        assert len(lines) == 1 and lines[0]["_type"] == "predict_video" and lines[0]["windows"] == 3
        recs[k] = lines[0]
    assert recs["entry"]["yuv_window"] == recs["flag"]["yuv_window"] == list(WINDOW) and "yuv_window" not in recs["tight"]
    assert recs["entry"]["shapes"]["overlay"] == [N, WINDOW[2], WINDOW[3], 3]
    want = np.load(paths["tight"][1])
    for k in ("entry", "flag"):
        z = np.load(paths[k][1])
        assert sorted(z.files) == sorted(want.files + ["yuv_window"])
        assert z["yuv_window"].tolist() == list(WINDOW)
        for name in want.files:
            assert z[name].dtype == want[name].dtype and np.array_equal(z[name], want[name], equal_nan=z[name].dtype.kind == "f"), name


def test_a_window_needs_frames_yuv_and_must_fit(tmp_path):
    video = str(tmp_path / "rgb.npz")
    np.savez(video, frames_u8=np.zeros((N, 64, 80, 3), np.uint8), wav=np.zeros(N * 800, np.float32))
    p = _run(video, str(tmp_path / "o.npz"), "--yuv-window", "0", "0", "32", "32")
    assert p.returncode != 0 and "holds no frames_yuv" in p.stderr and not os.path.exists(str(tmp_path / "o.npz"))
    video = str(tmp_path / "yuv.npz")
    np.savez(video, frames_yuv=np.zeros((N, HS * 3 // 2, WS), np.uint8), pixel_format=np.array("nv12"),
             wav=np.zeros(N * 800, np.float32))
    p = _run(video, str(tmp_path / "o.npz"), "--yuv-window", "4", "30", "64", "80")
    assert p.returncode != 0 and "exceeds the surface width" in p.stderr and not os.path.exists(str(tmp_path / "o.npz"))
