"""tools/predict.py --video --stream --chunk 13 --live hold --overlay --attention-track --attention-overlay mean in a child
process: the attention track folded from the streamed windows and the live_attention_* entries, with the shapes and dtypes the
tool documents; live_attention_frame is what csts_amd.live_attention_schedule states for the pushes the tool cuts."""
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
N, STRIDE, CHUNK, HW = 104, 9, 13, (64, 80)
OLD = ["points", "peak", "count", "rescaled", "heatmaps", "stream_windows", "stream_dropped"]
LIVE = ["live_points", "live_peak", "live_count", "live_known", "live_filled", "live_points_source", "live_overlay"]
TRACK = {"attention_maps": ((N, 9, 8, 8), np.float32), "attention_mixed": ((N, 9, 8, 8), np.float32),
         "attention_range": ((N, 9, 2), np.float32), "attention_count": ((N,), np.int32),
         "temporal_attention_windows": (None, np.float32)}
LIVE_ATTENTION = {"live_attention_frame": ((N,), np.int64), "live_attention_count": ((N,), np.int32),
                  "live_attention_maps": ((N, 9, 8, 8), np.float32), "live_attention_range": ((N, 9, 2), np.float32),
                  "live_attention_overlay": ((N,) + HW + (3,), np.uint8)}


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def test_stream_replay_writes_the_attention_track_and_the_live_attention(tmp_path):
    from csts_amd import live_attention_schedule, plan_stream
    from csts_amd.config import load_yaml
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N,) + HW + (3,), generator=g, dtype=torch.uint8)
    wav = 0.1 * torch.randn(N * 800 - 40, generator=g)
    video, out = str(tmp_path / "video.npz"), str(tmp_path / "live.npz")
    np.savez(video, frames_u8=frames.numpy(), wav=wav.numpy(), fps=np.float64(30.0))
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", str(STRIDE), "--stream", "--chunk",
                        str(CHUNK), "--out", out, "--live", "hold", "--overlay", "--attention-track", "--attention-overlay", "mean"]
                       + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(recs) == 1 and recs[0]["attention_track"] is True and recs[0]["live"] == "hold"
    z = np.load(out)
    assert sorted(z.files) == sorted(OLD + LIVE + list(TRACK) + list(LIVE_ATTENTION))
    for k, (shape, dt) in {**TRACK, **LIVE_ATTENTION}.items():
        assert z[k].dtype == dt and (shape is None or z[k].shape == shape), (k, z[k].shape, z[k].dtype)
    windows = len(z["stream_windows"])
    assert z["temporal_attention_windows"].shape[0] == windows >= 3 and recs[0]["attention_frames"] == int((z["attention_count"] > 0).sum())
    # the pushes the tool cuts: CHUNK frames with the samples up to their end, the rest with the last push
    pushes, sent = [], 0
    for a in range(0, N, CHUNK):
        b = min(a + CHUNK, N)
        upto = wav.numel() if b == N else min(wav.numel(), b * 800)
        pushes.append((b - a, upto - sent))
        sent = upto
    plan = plan_stream(load_yaml(YAML, ["NUM_GPUS", 0]), fps=30, stride=STRIDE)
    schedule = live_attention_schedule(plan, pushes)
    assert z["live_known"].tolist() == [kn for kn, _ in schedule]
    assert z["live_attention_frame"].tolist() == [g for _, g in schedule]
    held = z["live_attention_frame"] >= 0
    assert 0 < int(held.sum()) < N and (z["live_attention_count"][~held] == 0).all() and (z["live_attention_count"][held] > 0).all()
    assert np.isnan(z["live_attention_range"][~held]).all() and not np.isnan(z["live_attention_range"][held]).any()
    assert np.array_equal(z["live_attention_overlay"][~held], frames.numpy()[~held])
    assert not np.array_equal(z["live_attention_overlay"][held], frames.numpy()[held])
    # a frame the live row holds at age 0 whose windows had all run by then carries the folded track's own map
    final = [n for n in range(N) if held[n] and z["live_attention_frame"][n] == n and z["live_attention_count"][n] == z["attention_count"][n]]
    assert final
    for n in final:
        assert z["live_attention_maps"][n].tobytes() == z["attention_maps"][n].tobytes()

