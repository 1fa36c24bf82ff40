"""The host rules GazeStream, GazeStreamGroup and GazeLiveGroup share (csts_amd/stream.py), on CPU tensors (no GPU): the audio
tail step against a brute-force walk over the waveform, the closing windows and the dropped count against stream_schedule, the
K = 0 live dict, and the live / overlay arguments through both constructors."""
import itertools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EGO4D = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ESTIMATION = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Estimation.yaml")
HOP, N_FFT = 120, 511                                            # column f reads the samples [120 f - 120, 120 f + 120)


def _cfg(path):
    from csts_amd import load_yaml
    return load_yaml(path, ["NUM_GPUS", 0])


class _NoPredictor:
    """What the constructors read of a predictor before they allocate anything: its configuration."""
    def __init__(self, cfg):
        self.cfg = cfg


def _pieces(n, cut):
    if cut == "single":
        return [n]
    if cut == "ones":
        return [1] * n
    sizes, cycle = [], itertools.cycle((7, 113, 2000))
    while sum(sizes) < n:
        sizes.append(min(next(cycle), n - sum(sizes)))
    return sizes


@pytest.mark.parametrize("ring_cols", [832, 8])                  # the Ego4D ring, and one a 2000-sample piece overruns twice
@pytest.mark.parametrize("cut", ["single", "ones", "mixed"])
@pytest.mark.parametrize("n", [0, 1, 119, 120, 121, 511, 5000])
def test_audio_tail_step_against_a_walk_over_the_waveform(n, cut, ring_cols):
    from csts_amd.stream import audio_tail_step
    wav = torch.arange(1, n + 1, dtype=torch.float32)           # the first pushed sample is number 1
    samples = cols = base = at = 0
    tail, computed = None, []

    def step(piece, n_total):
        nonlocal samples, cols, tail, base
        old_base, old_cols = base, cols
        samples, cols, tail, base, buf, ranges = audio_tail_step(samples, cols, tail, old_base, piece, n_total, ring_cols)
        assert torch.equal(buf, wav[old_base:samples])          # the buffer is the waveform from the old tail on
        for f0, f1 in ranges:
            assert f0 < f1 <= f0 + ring_cols                    # at most one turn of the ring per launch
            assert max(0, HOP * f0 - HOP) >= old_base           # the buffer holds the first sample the range reads
            if n_total < 0:
                assert HOP * (f1 - 1) + HOP - 1 < samples      # and, while the signal runs, the last one
            computed.extend(range(f0, f1))
        assert cols == (old_cols if not ranges else ranges[-1][1])
        assert base <= max(0, HOP * cols - HOP)                 # the tail starts at or before the first sample column `cols` reads
        assert base + tail.numel() == samples and torch.equal(tail, wav[base:samples])
        assert tail.numel() < N_FFT + HOP

    for m in _pieces(n, cut):
        step(wav[at:at + m], -1)
        at += m
        assert cols == samples // HOP
    if tail is not None:                                         # close(): the column the offline STFT adds
        step(tail[:0], samples)
    want = 1 + (n + 2 * 255 - N_FFT) // HOP if tail is not None else 0      # n = 0: no column, with or without an empty piece
    assert samples == n and cols == want and computed == list(range(want))  # disjoint, ascending, every column once


@pytest.fixture(scope="module")
def plan():
    from csts_amd import plan_stream
    return plan_stream(_cfg(EGO4D), stride=9)


# window w needs 86 + 9 w frames and 120 * (572 + 60 w) samples: 104 frames run windows 0..2, 131 run 0..5, 140 run 0..6
@pytest.mark.parametrize("frames", [0, 22, 23, 85, 86, 103, 104, 131, 139, 140])
def test_closing_windows_and_dropped_against_stream_schedule(plan, frames):
    from csts_amd import stream_schedule
    from csts_amd.stream import closing_windows, dropped_windows
    edges = [120 * (572 + 60 * w) for w in (0, 2, 5, 6)]
    for samples in [0, 1, 5000] + [e + d for e in edges for d in (-120, -119, -1, 0, 1, 119)]:
        pushed = stream_schedule(plan, [(frames, samples)])[0]
        cols = 1 + (samples + 2 * 255 - N_FFT) // HOP           # after the padded last column
        closing = closing_windows(plan, len(pushed), frames, cols)
        # the closing rule is the schedule's with the samples rounded up to the padded column
        assert pushed + closing == stream_schedule(plan, [(frames, HOP * cols)])[0], (frames, samples)
        assert closing_windows(plan, len(pushed), frames, cols, started=False) == []
        ran = len(pushed) + len(closing)
        began = sum(1 for w in range(ran, 40) if 22 + 9 * w < frames)          # the first input frame of window w is 22 + 9 w
        assert dropped_windows(plan, ran, frames) == began, (frames, samples)
    assert dropped_windows(plan, 0, 104) == 10 and dropped_windows(plan, 3, 104) == 7


def test_closing_flush_is_what_the_spectrum_ring_still_takes(plan):
    from csts_amd.stream import closing_flush, ring_limits, stream_window
    limit = ring_limits(stream_window(plan, 0), 118, 832)[1]
    assert limit == 120 * 831 + 119
    assert closing_flush(plan, 118, 832, 0, 0, 30) == 30
    assert closing_flush(plan, 118, 832, 0, limit - 9, 30) == 9
    assert closing_flush(plan, 118, 832, 0, limit + 5, 30) == 0
    assert closing_flush(plan, 118, 832, 2, limit + 5, 30) == 30   # window 2 starts 120 columns later


FIELDS = {"frame_idx": ((0,), torch.int64), "known": ((0,), torch.int32), "points": ((0, 2), torch.float32),
          "peak": ((0,), torch.float32), "count": ((0,), torch.int32), "neighbours": ((0, 2), torch.int32),
          "filled": ((0,), torch.bool), "rescaled": ((0, 64, 64), torch.float32), "points_source": ((0, 2), torch.float64)}


@pytest.mark.parametrize("hw, overlay_format, shape", [((1080, 1088), None, (0, 1080, 1088, 3)), ((1080, 1088), "nv12", (0, 1620, 1088)),
                                                       (None, None, (0, 0, 0, 3)), (None, "nv12", (0, 0, 0))])
def test_the_live_dict_of_no_frames(hw, overlay_format, shape):
    from csts_amd.stream import live_empty
    plain = live_empty(64, "cpu", hw)
    assert list(plain) == list(FIELDS)
    for k, (s, dt) in FIELDS.items():
        assert tuple(plain[k].shape) == s and plain[k].dtype == dt, k
    drawn = live_empty(64, "cpu", hw, overlay=True, overlay_format=overlay_format)
    assert list(drawn) == list(FIELDS) + ["overlay"]
    assert tuple(drawn["overlay"].shape) == shape and drawn["overlay"].dtype == torch.uint8


def test_live_fields_and_the_batch_helpers():
    from csts_amd.stream import live_fields, pad_rows, window_result
    rows = {"count": torch.tensor([2, 0, 0], dtype=torch.int32), "neighbours": torch.tensor([[0, 0], [0, 3], [-1, -1]], dtype=torch.int32)}
    got = live_fields(rows, torch.arange(3), torch.full((3,), 4, dtype=torch.int32))
    assert got is rows and rows["filled"].tolist() == [False, True, False]     # predicted, filled, unpredicted
    assert rows["frame_idx"].tolist() == [0, 1, 2] and rows["known"].tolist() == [4, 4, 4]
    assert pad_rows([1, 2], 4) == [1, 2, 2, 2] and pad_rows([1, 2], 2) == [1, 2]
    out = {k: torch.arange(3) for k in ("points", "peak", "heatmaps", "rescaled")}
    r = {"window": 5, "frames_idx": "f", "target_idx": "t", "audio_centers": None}
    assert list(window_result(r, out, 1)) == ["window", "frames_idx", "target_idx", "points", "peak", "heatmaps", "rescaled"]
    grouped = window_result(r, out, 2, stream=7)
    assert list(grouped)[0] == "stream" and grouped["stream"] == 7 and grouped["window"] == 5 and int(grouped["peak"]) == 2


BAD = [({"live": "nearest"}, "live must be"), ({"alpha": 1.5, "overlay": True}, "alpha must lie in"), ({"radius": -1}, "radius"),
       ({"max_gap": 0}, "max_gap must be positive"), ({"overlay_format": "nv12"}, "pass overlay=True"),
       ({"overlay": True, "overlay_format": "nv12"}, "packed RGB"), ({"overlay": True, "overlay_format": "bgr"}, "overlay_format must be"),
       ({"overlay": True, "overlay_format": "i420", "pixel_format": "nv12"}, "layout of the frames")]


@pytest.mark.parametrize("kw, word", BAD)
def test_live_and_overlay_arguments_are_refused_alike_by_both_constructors(kw, word):
    from csts_amd import GazeLiveGroup, GazeStream
    cfg = _cfg(EGO4D)
    kw = dict({"live": "hold"}, **kw)
    with pytest.raises(ValueError, match=word) as single:
        GazeStream(_NoPredictor(cfg), **kw)
    with pytest.raises(ValueError, match=word) as group:         # refused before the arenas are allocated: no device needed
        GazeLiveGroup(_NoPredictor(cfg), 2, **kw)
    if kw["live"] == "hold":                                     # a GazeStream also takes live=None, and says so
        assert str(single.value) == str(group.value)


def test_check_live_args_results_and_the_estimation_plan():
    from csts_amd import GazeLiveGroup, GazeStream, plan_stream
    from csts_amd.stream import check_live_args
    plan = plan_stream(_cfg(EGO4D), stride=9)
    assert check_live_args(plan, 32, 256, {}, "hold", None, False, 0.4, 5, None) == (9, None, 104, 104 * (64 * 64 * 4 + 12))
    assert check_live_args(plan, 8, 256, {}, "linear", 4, True, 0.0, 0, "rgb24", required=True) == (4, None, 75, 75 * (64 * 64 * 4 + 12))
    assert check_live_args(plan, 32, 256, {"pixel_format": "nv12"}, "hold", None, True, 1.0, 5, "nv12")[1] == "nv12"
    assert check_live_args(plan, 32, 256, {}, None, None, False, 0.4, 5, None) == (None, None, 0, 0)
    with pytest.raises(ValueError, match="live must be one of"):
        check_live_args(plan, 32, 256, {}, None, None, False, 0.4, 5, None, required=True)
    for kw, word in (({"overlay": True}, "overlay=True.*needs live"), ({"max_gap": 4}, "max_gap.*needs live")):
        with pytest.raises(ValueError, match=word):
            GazeStream(_NoPredictor(_cfg(EGO4D)), **kw)
    est = _cfg(ESTIMATION)
    with pytest.raises(ValueError, match="already seen") as single:
        GazeStream(_NoPredictor(est), live="hold")
    with pytest.raises(ValueError, match="already seen") as group:
        GazeLiveGroup(_NoPredictor(est), 2, "hold")
    assert str(single.value) == str(group.value)
