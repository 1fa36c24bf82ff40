"""tools/predict.py --video on an nv12 recording with --overlay --overlay-format nv12, in a child process: the overlay in --out
is in the recording's layout, (N, H * 3 / 2, W), --out names it (overlay_pixel_format), every other entry is that of the run
without the flag, and --overlay-dir writes PNGs that are inputs.yuv_to_rgb_host of the overlay frames."""
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


def test_overlay_format_nv12(tmp_path):
    g = torch.Generator().manual_seed(21)
    yuv = torch.randint(0, 256, (N, H * 3 // 2, W), generator=g, dtype=torch.uint8).numpy()
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).numpy()
    video, out, pngs = str(tmp_path / "nv12.npz"), str(tmp_path / "track.npz"), tmp_path / "png"
    np.savez(video, frames_yuv=yuv, pixel_format=np.array("nv12"), wav=wav)
    cmd = [sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", "16", "--overlay", "--overlay-format", "nv12",
           "--overlay-dir", str(pngs), "--overlay-every", "40", "--out", out]
    p = subprocess.run(cmd + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(lines) == 1 and lines[0]["_type"] == "predict_video" and lines[0]["windows"] == 3
    assert lines[0]["pixel_format"] == "nv12" and lines[0]["shapes"]["overlay"] == [N, H * 3 // 2, W]
    z = np.load(out)
    assert str(z["overlay_pixel_format"]) == "nv12"
    assert z["overlay"].shape == (N, H * 3 // 2, W) and z["overlay"].dtype == np.uint8
    assert z["points_source"].shape == (N, 2) and z["rescaled"].shape == (N, 64, 64)
    drawn = z["count"] > 0
    assert 0 < drawn.sum() < N
    assert np.array_equal(z["overlay"][~drawn], yuv[~drawn]) and (z["overlay"][drawn] != yuv[drawn]).any()
    names = sorted(os.listdir(pngs)) if os.path.isdir(pngs) else []
    try:
        from PIL import Image
    except ImportError:
        assert names == [] and "PIL is not installed" in p.stdout
        return
    assert names == ["frame_000000.png", "frame_000040.png", "frame_000080.png"]
    for i in (0, 80):
        with Image.open(pngs / f"frame_{i:06d}.png") as im:
            assert im.size == (W, H) and im.mode == "RGB"
            assert np.array_equal(np.asarray(im), inputs.yuv_to_rgb_host(z["overlay"][i], "nv12"))
    # a layout the recording does not have is refused before the model is built
    bad = subprocess.run(cmd[:cmd.index("--overlay-format") + 1] + ["i420", "--out", str(tmp_path / "bad.npz")] + OPTS, cwd=ROOT,
                         env=_env(), capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--overlay-format i420" in bad.stderr and not os.path.exists(str(tmp_path / "bad.npz"))
