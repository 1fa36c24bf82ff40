"""tools/predict.py --video --stream on a recording whose npz carries sample_rate = 48000, in a child process: the audio is pushed
at 48 kHz and resampled inside the stream; the npz records both rates and the track is that of the same replay through the API."""
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
OPTS = ["NUM_GPUS", "1", "CSTS_AMD.COMPUTE", "bf16"]
PREDICT = os.path.join(ROOT, "tools", "predict.py")
N, STRIDE, CHUNK, RATE = 104, 9, 8, 48000


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def test_stream_replay_at_48_khz_writes_the_track_of_the_api_run(tmp_path):
    from csts_amd import GazePredictor, track_from_windows
    from csts_amd.config import assert_and_infer_cfg, load_yaml
    g = torch.Generator().manual_seed(22)
    frames = torch.randint(0, 256, (N, 64, 80, 3), generator=g, dtype=torch.uint8)
    wav = 0.1 * torch.randn(N * 1600 - 90, generator=g)          # 83 155 samples at 24 kHz: no multiple of the hop
    video, out = str(tmp_path / "v.npz"), str(tmp_path / "track.npz")
    np.savez(video, frames_u8=frames.numpy(), wav=wav.numpy(), fps=np.float64(30.0), sample_rate=np.int64(RATE))
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stream", "--chunk", str(CHUNK), "--stride",
                        str(STRIDE), "--out", out] + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(recs) == 1 and recs[0]["stream"] is True and recs[0]["chunk"] == CHUNK
    assert recs[0]["sample_rate"] == RATE and recs[0]["audio_rate"] == 24000 and recs[0]["windows"] == 3
    z = np.load(out)
    assert sorted(z.files) == sorted(["points", "peak", "count", "rescaled", "heatmaps", "stream_windows", "stream_dropped",
                                      "sample_rate", "audio_rate"])
    assert int(z["sample_rate"]) == RATE and int(z["audio_rate"]) == 24000
    assert z["stream_windows"].tolist() == [0, 1, 2]

    # the same replay through the API: the child seeds torch with cfg.RNG_SEED before it builds the model
    cfg = assert_and_infer_cfg(load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"]))
    dev = torch.device("cuda:0")
    torch.manual_seed(cfg.RNG_SEED)
    stream = GazePredictor(cfg, device=dev, graph=True).stream(fps=30, stride=STRIDE, input_rate=RATE)
    frames, wav = frames.to(dev), wav.to(dev)
    results, sent = [], 0
    for a in range(0, N, CHUNK):
        b = min(a + CHUNK, N)
        upto = wav.numel() if b == N else min(wav.numel(), b * 1600)
        results += stream.push(frames[a:b], wav[sent:upto] if upto > sent else None)
        sent = upto
    results += stream.close()
    track = track_from_windows(results, N)
    assert [r["window"] for r in results] == [0, 1, 2] and int(z["stream_dropped"]) == stream.dropped
    covered = z["count"] > 0
    assert np.array_equal(z["count"], track["count"].cpu().numpy()) and 0 < int(covered.sum()) < N
    assert np.array_equal(z["points"][covered], track["points"].cpu().numpy()[covered])
    assert np.isnan(z["points"][~covered]).all()
