"""GazeStream(live=...) against the offline composition it is defined by: the live row of frame f is row f of
fill_track(track_from_windows(results[:known(f)], f + max_gap + 1), mode, max_gap), bit for bit, and the overlay is
ops.gaze_overlay of the pushed frames with those rows and render_track's marker centres.  Random weights, bf16, the Ego4D forecast
YAML; 104 frames of 64 x 80 with 83 200 samples, stride 9: windows 0..2 (the fixture of tests/test_gpu_stream.py, restated)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import (GazePredictor, fill_track, inputs, marker_centers, ops, points_to_source, stream_live_schedule,  # noqa: E402
                      stream_window, track_from_windows)
from csts_amd.config import load_yaml  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, PER, S = 104, 64, 80, 9, 800, 256
WINDOW_KEYS = ("points", "peak", "heatmaps", "rescaled")
ROW_KEYS = ("points", "peak", "count", "neighbours", "filled", "rescaled")
CUTS = {"one_push": [(N, N * PER)],
        "thirteens": [(13, 13 * PER)] * 8,
        "uneven": [(0, 20 * PER), (1, PER), (5, 0), (40, 30 * PER), (11, 11 * PER), (32, 22 * PER), (2, 0), (13, 20 * PER)]}


def bits(a, b):
    """Exact equality: floats by bit pattern (the NaN points of unpredicted frames included), everything else by value."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    if a.dtype == torch.float64:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


@pytest.fixture(scope="module")
def env():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    g = torch.Generator().manual_seed(33)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    wav = (0.1 * torch.randn(N * PER, generator=g)).to(DEV)
    return {"cfg": cfg, "predictor": predictor, "frames": frames, "wav": wav, "plan": predictor.stream(stride=STRIDE).plan,
            "row": predictor._video_params_row(H, W)}


def replay(stream, pushes, frames, wav, live=True):
    """Push the counts in order -> (the windows, the per-push live dicts or None)."""
    fa = sa = 0
    windows, lives = [], []
    for k, m in pushes:
        f, a = (frames[fa:fa + k] if k else None), (wav[..., sa:sa + m] if m else None)
        if live:
            res, rows = stream.push_live(f, a)
            assert rows["frame_idx"].tolist() == list(range(fa, fa + k)) and rows["known"].dtype == torch.int32
            lives.append(rows)
        else:
            res = stream.push(f, a)
        windows += res
        fa, sa = fa + k, sa + m
    assert fa == frames.shape[0] and sa == wav.shape[-1]
    return windows, lives


def joined(lives):
    return {k: torch.cat([r[k] for r in lives], dim=0) for k in lives[0]}


def offline_row(windows, known, f, mode, max_gap):
    """Row f of the rule: fill_track(track_from_windows(results[:known], f + max_gap + 1)), or the unpredicted row for known 0."""
    if known == 0:
        return {"points": torch.full((2,), float("nan"), device=DEV), "peak": torch.zeros((), device=DEV),
                "count": torch.zeros((), dtype=torch.int32, device=DEV), "neighbours": torch.full((2,), -1, dtype=torch.int32, device=DEV),
                "filled": torch.zeros((), dtype=torch.bool, device=DEV), "rescaled": torch.zeros(S // 4, S // 4, device=DEV)}
    track = fill_track(track_from_windows(windows[:known], f + max_gap + 1), mode=mode, max_gap=max_gap)
    return {k: track[k][f] for k in ROW_KEYS}


def host_categories(plan, known, max_gap):
    """From the schedule alone: per frame "predicted", "filled" or "unpredicted"."""
    out = []
    for f, kn in enumerate(known):
        hit = sorted({int(t) for w in range(kn) for t in stream_window(plan, w)["target_idx"]})
        below, above = [t for t in hit if t < f], [t for t in hit if t > f]
        if f in hit:
            out.append("predicted")
        elif below and above and above[0] - below[-1] <= max_gap:
            out.append("filled")
        else:
            out.append("unpredicted")
    return out


@pytest.mark.parametrize("mode", ["hold", "linear"])
@pytest.mark.parametrize("cut", list(CUTS))
def test_live_rows_equal_the_offline_composition(env, cut, mode):
    pushes = CUTS[cut]
    assert sum(p[0] for p in pushes) == N and sum(p[1] for p in pushes) == N * PER
    s = env["predictor"].stream(stride=STRIDE, live=mode)
    assert s.max_gap == 9 and s.capacity["track_slots"] == 104
    windows, lives = replay(s, pushes, env["frames"], env["wav"])
    plain, _ = replay(env["predictor"].stream(stride=STRIDE), pushes, env["frames"], env["wav"], live=False)
    assert [r["window"] for r in windows] == [0, 1, 2] == [r["window"] for r in plain]
    for a, b in zip(windows, plain):                             # live on: the windows keep their bits
        for k in WINDOW_KEYS:
            assert bits(a[k], b[k]), (a["window"], k)
    live = joined(lives)
    known = stream_live_schedule(env["plan"], pushes)
    assert live["known"].tolist() == known and live["frame_idx"].tolist() == list(range(N))
    assert tuple(live["rescaled"].shape) == (N, 64, 64) and tuple(live["points_source"].shape) == (N, 2)
    for f in range(N):
        want = offline_row(windows, known[f], f, mode, 9)
        for k in ROW_KEYS:
            assert bits(live[k][f], want[k]), (f, known[f], k)
    assert bits(live["points_source"], points_to_source(live["points"], env["row"], S))
    kinds = host_categories(env["plan"], known, 9)
    assert [("predicted" if c > 0 else "filled" if fl else "unpredicted")
            for c, fl in zip(live["count"].tolist(), live["filled"].tolist())] == kinds
    if cut == "thirteens":       # frames 78..90 know window 0: 86 predicted, 87..90 filled, 78..85 not; 95 is predicted twice
        assert known[78:91] == [1] * 13 and known[91:] == [3] * 13 and known[:78] == [0] * 78
        assert kinds[86] == "predicted" and kinds[87:91] == ["filled"] * 4 and kinds[78:86] == ["unpredicted"] * 8
        assert int(live["count"][95]) == 2 and {"predicted", "filled", "unpredicted"} == set(kinds)
        if mode == "linear":
            assert not bits(live["rescaled"][88], live["rescaled"][87])
        else:
            assert bits(live["rescaled"][88], live["rescaled"][86]) and live["neighbours"][88].tolist() == [86, 95]


def test_overlay_is_gaze_overlay_of_the_pushed_frames_with_the_live_rows(env):
    p, frames = env["predictor"], env["frames"]
    s = p.stream(stride=STRIDE, live="linear", overlay=True, alpha=0.5, radius=3)
    _, lives = replay(s, CUTS["thirteens"], frames, env["wav"])
    live = joined(lives)
    assert live["overlay"].dtype == torch.uint8 and tuple(live["overlay"].shape) == (N, H, W, 3)
    params = torch.tensor(env["row"], dtype=torch.int32, device=DEV)
    centers = marker_centers(points_to_source(live["points"], env["row"], S), H, W)
    want = ops.gaze_overlay(frames, live["rescaled"], params, S, centers=centers, alpha=0.5, radius=3)
    assert torch.equal(live["overlay"], want)
    nothing = live["neighbours"][:, 0] < 0
    assert 0 < int(nothing.sum()) < N
    assert torch.equal(live["overlay"][nothing], frames[nothing])            # an unpredicted frame comes back byte for byte
    assert not torch.equal(live["overlay"][~nothing], frames[~nothing])
    rows_only = joined(replay(p.stream(stride=STRIDE, live="linear"), CUTS["thirteens"], frames, env["wav"])[1])
    assert "overlay" not in rows_only
    for k in rows_only:                                                       # drawing changes no row
        assert bits(rows_only[k], live[k]), k


def test_nv12_stream_draws_on_the_converted_pictures(env):
    g = torch.Generator().manual_seed(35)
    yuv = torch.randint(0, 256, (N, H * 3 // 2, W), generator=g, dtype=torch.uint8).to(DEV)
    fmt = {"pixel_format": "nv12", "matrix": "bt709", "full_range": False}
    rgb = inputs.yuv_to_rgb(yuv, **fmt)
    a = joined(replay(env["predictor"].stream(stride=STRIDE, live="hold", overlay=True, **fmt), CUTS["thirteens"], yuv, env["wav"])[1])
    b = joined(replay(env["predictor"].stream(stride=STRIDE, live="hold", overlay=True), CUTS["thirteens"], rgb, env["wav"])[1])
    assert tuple(a["overlay"].shape) == (N, H, W, 3) and int((a["count"] > 0).sum()) > 0
    for k in a:
        assert bits(a[k], b[k]), k
    nothing = a["neighbours"][:, 0] < 0
    assert torch.equal(a["overlay"][nothing], rgb[nothing]) and not torch.equal(a["overlay"][~nothing], rgb[~nothing])


def test_input_rate_48000_gives_the_rows_of_the_resampled_waveform(env):
    g = torch.Generator().manual_seed(36)
    wav48 = (0.1 * torch.randn(N * 2 * PER, generator=g)).to(DEV)
    whole = inputs.resample_audio(wav48, 48000)
    _, up, down, half = inputs.resample_rule(48000)
    pushes48 = [(13, 13 * 2 * PER)] * 8
    ends = np.cumsum([m for _, m in pushes48])
    final = [inputs.resample_ready(int(e), up, down, half) for e in ends]   # the 24 kHz samples final after each push
    pushes24 = [(13, b - a) for a, b in zip([0] + final[:-1], final)]
    win48, lives48 = replay(env["predictor"].stream(stride=STRIDE, live="linear", input_rate=48000), pushes48, env["frames"], wav48)
    win24, lives24 = replay(env["predictor"].stream(stride=STRIDE, live="linear"), pushes24, env["frames"], whole[:final[-1]])
    a, b = joined(lives48), joined(lives24)
    assert a["known"].tolist() == stream_live_schedule(env["plan"], pushes48, input_rate=48000) == b["known"].tolist()
    assert [r["window"] for r in win48] == [r["window"] for r in win24] and len(win48) >= 2 and int((a["count"] > 0).sum()) > 0
    for k in a:
        assert bits(a[k], b[k]), k


def test_without_live_nothing_changes_and_push_live_raises(env):
    s = env["predictor"].stream(stride=STRIDE)
    assert s.live is None and "track_slots" not in s.capacity and s._track is None
    with pytest.raises(ValueError, match="open the stream with live"):
        s.push_live(env["frames"][:1])
    assert (s.frames, s.samples) == (0, 0)
    res = s.push(env["frames"], env["wav"])
    assert s._track is None
    # push() on a live stream returns the same windows, and what it ran is in the ring for a later push_live
    live = env["predictor"].stream(stride=STRIDE, live="hold")
    again = live.push(env["frames"][:100], env["wav"])
    both, rows = live.push_live(env["frames"][100:], None)
    assert [r["window"] for r in again + both] == [0, 1, 2] == [r["window"] for r in res]
    for a, b in zip(again + both, res):
        for k in WINDOW_KEYS:
            assert bits(a[k], b[k]), (a["window"], k)
    assert rows["frame_idx"].tolist() == [100, 101, 102, 103] and rows["known"].tolist() == [3] * 4
    for i, f in enumerate(range(100, 104)):
        want = offline_row(res, 3, f, "hold", 9)
        for k in ROW_KEYS:
            assert bits(rows[k][i], want[k]), (f, k)
    none, empty = live.push_live(None, env["wav"][:0])                       # a push without frames answers no frame
    assert none == [] and empty["frame_idx"].numel() == 0 and tuple(empty["rescaled"].shape) == (0, 64, 64)
