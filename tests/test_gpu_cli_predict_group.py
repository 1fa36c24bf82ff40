"""tools/predict.py --videos A B --stream --chunk 8 --batch 2 in a child process: two recordings replayed as the slots of one
GazeStreamGroup; the two files it writes hold the windows group_schedule predicts, the batches each slot took part in, and the
points of the same replay done through the API in this process."""
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
STRIDE, CHUNK, BATCH = 9, 8, 2
SHAPES = [(104, 64, 80, 104 * 800 - 40), (95, 48, 64, 95 * 800)]   # slot 0: no multiple of the hop, close() adds a column


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _ticks():
    """The (frames, samples) counts the tool pushes: chunks of CHUNK frames with the samples up to their last frame, the rest of
    the waveform with the last chunk."""
    ticks, sent = [], [0, 0]
    for a in range(0, 104, CHUNK):
        tick = {}
        for i, (N, _, _, n) in enumerate(SHAPES):
            if a < N:
                b = min(a + CHUNK, N)
                upto = n if b == N else min(n, b * 800)
                tick[i], sent[i] = (b - a, upto - sent[i]), upto
        ticks.append(tick)
    return ticks


def test_two_recordings_replayed_as_one_group_write_the_windows_of_the_schedule(tmp_path):
    from csts_amd import GazePredictor, group_schedule, track_from_windows
    from csts_amd.config import assert_and_infer_cfg, load_yaml
    g = torch.Generator().manual_seed(23)
    recs, paths = [], []
    for i, (N, H, W, n) in enumerate(SHAPES):
        recs.append((torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8), 0.1 * torch.randn(n, generator=g)))
        paths.append(str(tmp_path / f"video{i}.npz"))
        np.savez(paths[-1], frames_u8=recs[-1][0].numpy(), wav=recs[-1][1].numpy(), fps=np.float64(30.0))
    out = str(tmp_path / "track.npz")
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--videos", *paths, "--stride", str(STRIDE), "--stream", "--chunk",
                        str(CHUNK), "--batch", str(BATCH), "--out", out] + OPTS, cwd=ROOT, env=_env(), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    recs_out = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert [r["stream_slot"] for r in recs_out] == [0, 1] and all(r["stream"] is True and r["batch"] == BATCH for r in recs_out)
    assert [r["windows"] for r in recs_out] == [3, 2] and [r["dropped"] for r in recs_out] == [7, 7]
    assert not os.path.exists(out)

    cfg = assert_and_infer_cfg(load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"]))
    dev = torch.device("cuda:0")
    torch.manual_seed(cfg.RNG_SEED)                               # the child seeds torch with cfg.RNG_SEED before it builds the model
    group = GazePredictor(cfg, device=dev, graph=True).stream_group(2, fps=30, stride=STRIDE, batch=BATCH)
    ticks = _ticks()
    schedule = group_schedule(group.plan, ticks, BATCH)
    batches = [rows for tick in schedule for rows in tick]
    assert batches == [[(0, 0), (1, 0)], [(0, 1), (1, 1)], [(0, 2)]]
    results, at = [[], []], [[0, 0], [0, 0]]
    for tick, want in zip(ticks, schedule):
        pieces = {}
        for i, (k, m) in tick.items():
            frames, wav = recs[i]
            pieces[i] = (frames[at[i][0]:at[i][0] + k].to(dev), wav[at[i][1]:at[i][1] + m].to(dev) if m else None)
            at[i] = [at[i][0] + k, at[i][1] + m]
        for i, rs in group.push(pieces).items():
            results[i] += rs
        assert group.batches == want
        for i in tick:
            if at[i][0] == SHAPES[i][0]:
                assert group.close(i) == {i: []} and group.batches == []     # the padded column completes no further window
    assert group.closed == [True, True] and group.dropped == [7, 7]

    for i, (N, _, _, _) in enumerate(SHAPES):
        z = np.load(str(tmp_path / f"track_{i}.npz"))
        assert sorted(z.files) == sorted(["points", "peak", "count", "rescaled", "heatmaps", "stream_windows", "stream_dropped",
                                          "stream_slot", "stream_batches"])
        assert int(z["stream_slot"]) == i and int(z["stream_dropped"]) == 7
        assert z["stream_windows"].tolist() == [w for rows in batches for s, w in rows if s == i] == [r["window"] for r in results[i]]
        mine = [rows + [(-1, -1)] * (BATCH - len(rows)) for rows in batches if any(s == i for s, _ in rows)]
        assert z["stream_batches"].dtype == np.int64 and z["stream_batches"].tolist() == [[list(r) for r in rows] for rows in mine]
        assert z["points"].shape == (N, 2) and z["heatmaps"].shape == (N, 64, 64)
        track = track_from_windows(results[i], N)
        covered = z["count"] > 0
        assert np.array_equal(z["count"], track["count"].cpu().numpy()) and 0 < int(covered.sum()) < N
        assert np.array_equal(z["points"][covered], track["points"].cpu().numpy()[covered])
        assert np.isnan(z["points"][~covered]).all()


def test_videos_needs_stream_and_refuses_live_overlay_and_attention(tmp_path, capsys):
    a, b, out = str(tmp_path / "a.npz"), str(tmp_path / "b.npz"), str(tmp_path / "o.npz")
    p = subprocess.run([sys.executable, PREDICT, "--cfg", YAML, "--videos", a, b, "--out", out] + OPTS, cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and p.stdout.strip() == "" and "needs --stream" in p.stderr
    # the other refusals come from the same argument check: asked of it in this process (argparse exits with status 2)
    import importlib.util
    spec = importlib.util.spec_from_file_location("predict_tool", PREDICT)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for extra, word in (([], "needs --stream"), (["--stream", "--live", "hold"], "not part of a stream group"),
                        (["--stream", "--overlay"], "not part of a stream group"),
                        (["--stream", "--attention-track"], "not part of a stream group"),
                        (["--stream", "--attention"], "not part of a stream group"),
                        (["--stream", "--fill", "hold"], "not part of a stream group"),
                        (["--stream", "--video", a], "exclude each other")):
        with pytest.raises(SystemExit) as e:
            tool.parse_args(["--cfg", YAML, "--videos", a, b] + extra + ["--out", out] + OPTS)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    args = tool.parse_args(["--cfg", YAML, "--videos", a, b, "--stream", "--chunk", "8", "--batch", "2", "--out", out] + OPTS)
    assert args.videos == [a, b] and args.batch == 2 and args.opts == OPTS
