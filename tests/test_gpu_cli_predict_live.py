"""tools/predict.py --video --stream --chunk 13 --live linear --overlay in a child process: the live_* entries it writes are those
of the same replay through GazeStream.push_live in this process, and the entries a run without --live writes keep their bits."""
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
N, STRIDE, CHUNK = 104, 9, 13
OLD = ["points", "peak", "count", "rescaled", "heatmaps", "stream_windows", "stream_dropped"]
LIVE = ["live_points", "live_peak", "live_count", "live_known", "live_filled", "live_points_source", "live_overlay"]


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _run(video, out, extra):
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--video", video, "--stride", str(STRIDE), "--stream", "--chunk",
                        str(CHUNK), "--out", out] + extra + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert len(recs) == 1
    return recs[0], np.load(out)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()        # bytes: NaN points included


def test_live_replay_writes_the_rows_of_the_api_run(tmp_path):
    from csts_amd import GazePredictor, stream_live_schedule
    from csts_amd.config import assert_and_infer_cfg, load_yaml
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N, 64, 80, 3), generator=g, dtype=torch.uint8)
    wav = 0.1 * torch.randn(N * 800 - 40, generator=g)           # no multiple of the hop: close() adds a column
    video = str(tmp_path / "video.npz")
    np.savez(video, frames_u8=frames.numpy(), wav=wav.numpy(), fps=np.float64(30.0))
    rec, z = _run(video, str(tmp_path / "live.npz"), ["--live", "linear", "--overlay"])
    plain_rec, plain = _run(video, str(tmp_path / "plain.npz"), [])
    assert sorted(plain.files) == sorted(OLD) and sorted(z.files) == sorted(OLD + LIVE)
    for k in OLD:                                                # what a run without --live writes keeps its bits
        assert same(z[k], plain[k]), k
    assert rec["live"] == "linear" and rec["max_gap"] == 9 and rec["stream"] is True and rec["chunk"] == CHUNK
    assert "live" not in plain_rec and {k: v for k, v in rec.items() if k in plain_rec and k not in ("out", "shapes")} == \
        {k: v for k, v in plain_rec.items() if k not in ("out", "shapes")}
    assert rec["live_filled_frames"] == int(z["live_filled"].sum()) > 0

    # the same replay through the API: the child seeds torch with cfg.RNG_SEED before it builds the model
    cfg = assert_and_infer_cfg(load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"]))
    dev = torch.device("cuda:0")
    torch.manual_seed(cfg.RNG_SEED)
    stream = GazePredictor(cfg, device=dev, graph=True).stream(fps=30, stride=STRIDE, live="linear", overlay=True)
    frames, wav = frames.to(dev), wav.to(dev)
    rows, pushes, sent = [], [], 0
    for a in range(0, N, CHUNK):
        b = min(a + CHUNK, N)
        upto = wav.numel() if b == N else min(wav.numel(), b * 800)
        rows.append(stream.push_live(frames[a:b], wav[sent:upto] if upto > sent else None)[1])
        pushes.append((b - a, upto - sent))
        sent = upto
    live = {k: torch.cat([r[k] for r in rows]).cpu().numpy() for k in rows[0]}
    assert live["known"].tolist() == stream_live_schedule(stream.plan, pushes) == z["live_known"].tolist()
    for k in LIVE:
        assert same(z[k], live[k[len("live_"):]]), k
    assert z["live_overlay"].shape == (N, 64, 80, 3) and z["live_count"].dtype == np.int32 and z["live_filled"].dtype == np.bool_
    assert 0 < int((z["live_count"] > 0).sum()) < N and np.isnan(z["live_points"][z["live_known"] == 0]).all()
    nothing = np.isnan(z["live_points"][:, 0])
    assert np.array_equal(z["live_overlay"][nothing], frames.cpu().numpy()[nothing])


def test_live_needs_a_stream_and_leaves_fill_offline(tmp_path, capsys):
    """The argument rules, on the tool's own parser (no child process: nothing is loaded or run)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("predict_tool", PREDICT)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["--cfg", YAML, "--out", str(tmp_path / "o.npz"), "--video", str(tmp_path / "v.npz")]
    for extra, word in ((["--live", "hold"], "needs --stream"), (["--stream", "--overlay"], "not part"),
                        (["--stream", "--live", "hold", "--fill", "hold"], "not part"), (["--stream", "--max-gap", "4"], "needs --fill")):
        with pytest.raises(SystemExit):
            tool.parse_args(base + extra)
        assert word in capsys.readouterr().err, extra
    args = tool.parse_args(base + ["--stream", "--live", "linear", "--overlay", "--max-gap", "4"])
    assert (args.live, args.overlay, args.max_gap, args.fill) == ("linear", True, 4, None)
