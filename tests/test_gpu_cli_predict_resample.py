"""tools/predict.py --video on a recording whose npz carries sample_rate: the waveform is resampled on the device, --out records
sample_rate and audio_rate, the track is the API's, and --sample-rate overrides the entry.  The first run is a child process, the
command line proper; the override runs the tool's main() in this process, which spares a second interpreter start."""
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
OPTS = ["NUM_GPUS", "1", "TEST.BATCH_SIZE", "2", "CSTS_AMD.COMPUTE", "fp32"]
PREDICT = os.path.join(ROOT, "tools", "predict.py")
N, STRIDE = 200, 32
TRACK = ("points", "peak", "count", "rescaled", "heatmaps")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


class _NoOptimizer:
    def state_dict(self):
        return {}


def _run(video, out, *more):
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", str(STRIDE), "--out", out] + list(more) +
                       OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(recs) == 1 and recs[0]["_type"] == "predict_video"
    return recs[0], np.load(out)


def test_rate_entry_is_honoured_recorded_and_overridden(tmp_path, capsys):
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N, 64, 80, 3), generator=g, dtype=torch.uint8)
    wav = 0.1 * torch.randn(2, N * 48000 // 30, generator=g)
    video = str(tmp_path / "video.npz")
    np.savez(video, frames_u8=frames.numpy(), wav=wav.numpy(), fps=np.float64(30.0), sample_rate=np.int64(48000))
    # the weights both sides use: saved here, loaded by the child
    from csts_amd import GazePredictor, checkpoint as ck
    from csts_amd.config import assert_and_infer_cfg, load_yaml
    cfg = assert_and_infer_cfg(load_yaml(YAML, ["NUM_GPUS", 1] + OPTS[2:]))
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=dev)
    path = ck.save_checkpoint(str(tmp_path), predictor.model, _NoOptimizer(), 0, cfg)
    rec, z = _run(video, str(tmp_path / "track.npz"), "--checkpoint", path)
    assert rec["sample_rate"] == 48000 and rec["audio_rate"] == 24000 and rec["frames"] == N
    assert sorted(z.files) == sorted(TRACK + ("sample_rate", "audio_rate")) and sorted(rec["shapes"]) == sorted(TRACK)
    assert int(z["sample_rate"]) == 48000 and int(z["audio_rate"]) == 24000
    api = predictor.predict_video(frames.to(dev), wav.to(dev), fps=30.0, stride=STRIDE, sample_rate=48000)
    for k in TRACK:
        assert np.array_equal(z[k], api[k].cpu().numpy(), equal_nan=True), k
    # --sample-rate wins over the entry: the same samples read as 32 kHz stereo give another track and are recorded so
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import predict as tool
    capsys.readouterr()
    tool.main(["--cfg", YAML, "--video", video, "--stride", str(STRIDE), "--out", str(tmp_path / "track2.npz"), "--checkpoint", path,
               "--sample-rate", "32000"] + OPTS)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("json_stats: ")]
    assert len(lines) == 1
    rec2, z2 = json.loads(lines[0][len("json_stats: "):]), np.load(str(tmp_path / "track2.npz"))
    assert rec2["sample_rate"] == 32000 and int(z2["sample_rate"]) == 32000 and int(z2["audio_rate"]) == 24000
    assert not np.array_equal(z2["heatmaps"], z["heatmaps"])
    api2 = predictor.predict_video(frames.to(dev), wav.to(dev), fps=30.0, stride=STRIDE, sample_rate=32000)
    assert np.array_equal(z2["heatmaps"], api2["heatmaps"].cpu().numpy())
